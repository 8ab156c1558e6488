"""The bf16 mixed-precision training mode without a GPU: the new kernel file compiles for gfx950 without spills and really
is bf16 MFMA, the command lines and the constructors take `precision`, and checkpoints keep the reference's names."""
import glob
import os
import re
import subprocess

import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import nnet, reinforce, train
from conftest import REPO

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_bf16_kernels_build_without_spills_on_bf16_mfma(tmp_path):
    """bk_train_bf16.hip alone: zero VGPR / SGPR spills in every kernel; every conv kernel's ISA holds a bf16 MFMA and
    the file holds no fp32 one (the mode must not quietly be the fp32 kernel)."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "--save-temps",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_train_bf16.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    spills = re.findall(r"(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(kernels) >= 7 and len(spills) == 2 * len(kernels)
    assert all(int(n) == 0 for _, n in spills), spills

    isa = [p for p in glob.glob(str(tmp_path / "*.s")) if "gfx950" in os.path.basename(p)]
    assert len(isa) == 1, isa
    text = open(isa[0]).read()
    # one body per kernel: from its label to the .Lfunc_end that closes it
    bodies = dict(re.findall(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M))
    conv = {k: v for k, v in bodies.items() if re.search(r"conv_(fwd|wgrad)\d?_bf16_kernel", k)}
    assert len(conv) == 4, sorted(bodies)                       # forward and weight gradient, k = 5 and k = 3
    for name, body in conv.items():
        assert re.search(r"\bv_mfma_f32_\w+_bf16\b", body), name
        assert "v_mfma_f32_16x16x4_f32" not in body, name
        assert "v_cvt_pk_bf16_f32" in body, name                # operands are rounded in the kernel, RNE
    assert "v_mfma_f32_16x16x4_f32" not in text


def test_command_lines_take_precision(tmp_path, capsys):
    d = str(tmp_path)
    assert reinforce._parse(["-w", d, "--precision", "bf16"]).precision == "bf16"
    assert reinforce._parse(["-w", d]).precision == "fp32"
    with pytest.raises(SystemExit) as e:
        reinforce._parse(["-w", d, "--precision", "fp16"])
    assert e.value.code == 2 and "--precision" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        train.main(["--records", d, "--precision", "fp16"])
    assert e.value.code == 2 and "--precision" in capsys.readouterr().err


def test_bf16_nets_keep_the_checkpoint_names():
    counters = [f"conv.{b}.num_batches_tracked" for b in (1, 4, 7, 10, 13, 16, 19)]
    p = train.TrainablePolicyNet(device="cpu", precision="bf16")
    assert p.precision == "bf16"
    assert set(p.state_dict()) == set(nnet._TRUNK_NAMES) | set(counters)
    assert set(p.state_dict()) == set(train.TrainablePolicyNet(device="cpu").state_dict())
    v = train.TrainableValueNet(device="cpu", precision="bf16")
    assert v.precision == "bf16"
    assert set(v.state_dict()) == set(nnet._VALUE_NAMES) | set(counters) | {"bn.num_batches_tracked",
                                                                             "lin_bn.num_batches_tracked"}
    assert set(v.state_dict()) == set(train.TrainableValueNet(device="cpu").state_dict())
    assert train.TrainablePolicyNet(device="cpu").precision == "fp32"
    v2 = train.TrainableValueNet.from_state_dict(v.state_dict(), device="cpu", precision="bf16")
    assert v2.precision == "bf16" and all(torch.equal(a, v.state_dict()[k]) for k, a in v2.state_dict().items())
    for cls in (train.TrainablePolicyNet, train.TrainableValueNet):
        with pytest.raises(ValueError):
            cls(device="cpu", precision="fp16")


def test_binding_refuses_an_unknown_precision_first():
    """before it looks at the tensors or at the library: none of these arguments is a tensor"""
    for call in (lambda: T.conv_forward(None, None, precision="tf32"), lambda: T.conv_pack(None, precision="tf32"),
                 lambda: T.conv_dgrad(None, None, precision="tf32"),
                 lambda: T.conv_wgrad(None, None, None, precision="tf32")):
        with pytest.raises(ValueError, match="precision"):
            call()
    assert T.BKT_ABI_VERSION == 4
    for name in ("bkt_conv_packed_elems_bf16", "bkt_conv_pack_bf16", "bkt_conv_forward_bf16",
                 "bkt_conv_pack_dgrad_bf16", "bkt_conv_dgrad_bf16", "bkt_conv_wgrad_workspace_bf16",
                 "bkt_conv_wgrad_bf16"):
        assert name in T.SYMBOLS
