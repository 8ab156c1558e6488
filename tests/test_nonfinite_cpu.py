"""The float64 reference of tests/nonfinite_cases.py on its own: every case does something, and what it does has the shape
the contract quotes (include/bokego_train.h, "Non-finite values").  No GPU: this is what keeps test_gpu_nonfinite.py from
passing on an empty comparison."""
import math

import pytest
import torch

import nonfinite_cases as N


def _sets(case):
    """per output: (non-finite, finite and changed by the poison, finite and untouched) as boolean tensors"""
    ref, _ = N.case_reference(case)
    clean, _ = N.clean_reference(case)
    out = {}
    for name in N.OUTPUTS[case.setup.op]:
        a, b = ref[name], clean[name]
        if not a.dtype.is_floating_point:
            assert a.item() == b.item() == 1                    # num_batches_tracked counts the call, whatever x holds
            continue
        same = N.same_bits(a, b)
        out[name] = (~a.isfinite(), a.isfinite() & ~same, a.isfinite() & same)
    return out


def _no_effect(c):
    """Cases the reference is indifferent to, by construction: the ReLU is shut at "corner" (y = 0), so a gradient that
    arrives there is dropped whatever it is, and an x of -Inf there gives the 0 the clean call gives."""
    op = c.setup.op
    return c.where == "corner" and ((op in ("bn_relu_backward", "bn_relu_eval_backward") and c.operand == "dy") or
                                    (op == "bn_relu_eval" and c.operand == "x" and c.kind == "-inf"))


def _finite_effect(c):
    """Cases whose whole effect is finite: the poison moves a ReLU mask, or meets a 0 or an Inf that swallows it."""
    op, name, kind = c.setup.op, c.operand, c.kind
    if op == "bn_relu_train":              # relu(-Inf) is 0; sqrt is not taken of the running variance
        return (name == "beta" and kind == "-inf") or (name == "running_var" and kind == "-1")
    if op == "bn_relu_backward":           # beta reaches the gradients only through the mask [y > 0]
        return name == "beta"
    if op == "bn_relu_eval":               # relu(-Inf) is 0; a variance of +Inf is a scale of 0: y = relu(beta)
        return ((name in ("x", "beta") and kind == "-inf") or (name == "running_mean" and kind == "+inf") or
                (name == "running_var" and kind == "+inf"))
    if op == "bn_relu_eval_backward":      # the same through the mask; x = -Inf where the ReLU was open anyway shuts it
        return name == "beta" or (name == "running_var" and kind == "+inf")
    return False


@pytest.mark.parametrize("setup", N.setups(), ids=N.setup_id)
def test_every_case_does_something(setup):
    bad = []
    for c in N.cases(setup):
        sets = _sets(c)
        nonfinite = sum(int(s[0].sum()) for s in sets.values())
        changed = sum(int(s[1].sum()) for s in sets.values())
        untouched = sum(int(s[2].sum()) for s in sets.values())
        if untouched == 0:
            bad.append((N.case_id(c), "no finite element left to compare bit for bit"))
        if _no_effect(c):
            if nonfinite or changed:
                bad.append((N.case_id(c), "expected to leave every output as it is", nonfinite, changed))
        elif _finite_effect(c):
            if nonfinite or not changed:
                bad.append((N.case_id(c), "expected a finite effect only", nonfinite, changed))
        elif nonfinite == 0:
            bad.append((N.case_id(c), "no non-finite element in any output"))
        if setup.op.startswith("conv_") and changed:             # a convolution's finite outputs never saw the poison
            bad.append((N.case_id(c), "finite elements of a convolution changed", changed))
    assert not bad, bad


def test_the_clean_relu_is_open_and_shut_where_the_poison_goes():
    for setup in N.setups():
        if not setup.op.startswith("bn_"):
            continue
        _, hand = N.clean_reference(N.cases(setup)[0])
        y = hand["y"].reshape(-1)
        pos = N._positions("x", (setup.B, N.C, 9, 9))
        assert all(y[pos[w]] > 0 for w in ("first", "last", "centre")) and y[pos["corner"]] == 0, N.setup_id(setup)


def test_relu_reference():
    x = torch.tensor([N.NAN, N.INF, -N.INF], dtype=torch.float64, requires_grad=True)
    y = torch.relu(x)
    y.sum().backward()
    assert math.isnan(y[0].item()) and y[1].item() == N.INF and y[2].item() == 0
    assert x.grad.tolist() == [1.0, 1.0, 0.0]


def _case(setup, operand, where, kind):
    (c,) = [c for c in N.cases(setup) if (c.operand, c.where, c.kind) == (operand, where, kind)]
    return c


def _channel_of(index):
    return (index // 81) % N.C


@pytest.mark.parametrize("B", N.BATCHES)
@pytest.mark.parametrize("kind", list(N.KINDS))
@pytest.mark.parametrize("where", ["first", "last", "corner", "centre"])
def test_train_batchnorm_loses_the_whole_channel(B, where, kind):
    c = _case(N.Setup("bn_relu_train", B, N.C, 0), "x", where, kind)
    ref, _ = N.case_reference(c)
    sets = _sets(c)
    ch = _channel_of(c.index)
    want = torch.zeros((B, N.C, 9, 9), dtype=torch.bool)
    want[:, ch] = True
    assert torch.equal(ref["y"].isnan(), want) and not sets["y"][1].any()     # all B * 81 NaN, the other channels untouched
    rm, rv = ref["running_mean"], ref["running_var"]
    assert (math.isnan(rm[ch].item()) if kind == "nan" else rm[ch].item() == N.KINDS[kind]) and math.isnan(rv[ch].item())
    only = torch.arange(N.C) == ch
    for name in ("save_mean", "save_invstd", "running_mean", "running_var"):
        assert torch.equal(sets[name][0], only) and not sets[name][1].any(), name


@pytest.mark.parametrize("B", N.BATCHES)
@pytest.mark.parametrize("kind", list(N.KINDS))
@pytest.mark.parametrize("where", ["first", "last", "centre"])
def test_eval_batchnorm_keeps_it_to_the_element(B, where, kind):
    c = _case(N.Setup("bn_relu_eval", B, N.C, 0), "x", where, kind)
    ref, _ = N.case_reference(c)
    nonfinite, changed, _ = _sets(c)["y"]
    y = ref["y"].reshape(-1)
    at = torch.arange(y.numel()) == c.index
    if kind == "-inf":                                           # relu(-Inf): 0 where the clean call had y > 0
        assert y[c.index] == 0 and torch.equal(changed.reshape(-1), at) and not nonfinite.any()
    else:
        assert math.isnan(y[c.index].item()) if kind == "nan" else y[c.index].item() == N.INF
        assert torch.equal(nonfinite.reshape(-1), at) and not changed.any()


def _conv_setups(op):
    return [s for s in N.setups() if s.op == op]


@pytest.mark.parametrize("setup", _conv_setups("conv_forward"), ids=N.setup_id)
def test_convolution_sets(setup):
    B, cin, k = setup.B, setup.cin, setup.k
    # a NaN weight w[m, ci, tap]: all 81 points of channel m on every board, zero padding included, and nothing else
    for where, m in (("first", 0), ("last", N.C - 1)):
        ref, _ = N.case_reference(_case(setup, "w", where, "nan"))
        want = torch.zeros((B, N.C, 9, 9), dtype=torch.bool)
        want[:, m] = True
        assert torch.equal(ref["y"].isnan(), want)
        # ... and an Inf there is NaN exactly where its tap falls on the padding (Inf * 0), Inf elsewhere in the channel
        ref, _ = N.case_reference(_case(setup, "w", where, "+inf"))
        on = (9 - k // 2) ** 2                                   # points whose corner tap is on the board, per board
        assert torch.equal(~ref["y"].isfinite(), want) and int(ref["y"].isinf().sum()) == B * on
    # a NaN in x: the points within reach of it, in every channel of its board
    for where, points in (("first", (k // 2 + 1) ** 2), ("corner", (k // 2 + 1) ** 2), ("last", (k // 2 + 1) ** 2),
                          ("centre", k * k)):
        c = _case(setup, "x", where, "nan")
        nan = N.case_reference(c)[0]["y"].isnan()
        b = c.index // (cin * 81)
        assert int(nan.sum()) == points * N.C and int(nan[b].sum()) == points * N.C
        assert (nan[b].sum((1, 2)) == points).all()
    # Inf against a weight that is exactly 0: NaN in that channel, +-Inf in the others, at the point itself
    c = _case(setup, "x", "zero_weight", "+inf")
    y = N.case_reference(c)[0]["y"]
    assert math.isnan(y[0, N.ZERO_M, 4, 4].item()) and int(y.isnan().sum()) == 1
    assert int(y[0, :, 4, 4].isinf().sum()) == N.C - 1 and int(y.isinf().sum()) == k * k * N.C - 1


@pytest.mark.parametrize("setup", _conv_setups("conv_wgrad"), ids=N.setup_id)
def test_weight_gradient_sets(setup):
    # a NaN in dy[b, m, p]: all of dw[m] and db[m], no other row
    for where in ("first", "last", "corner", "centre"):
        c = _case(setup, "dy", where, "nan")
        ref, _ = N.case_reference(c)
        m = _channel_of(c.index)
        want = torch.zeros((N.C, setup.cin, setup.k, setup.k), dtype=torch.bool)
        want[m] = True
        assert torch.equal(ref["dw"].isnan(), want) and torch.equal(ref["db"].isnan(), torch.arange(N.C) == m)


@pytest.mark.parametrize("which", ["policy", "value"])
def test_a_nan_weight_reaches_the_loss_and_every_later_layer(which):
    loss, grads, bufs = N.step_reference(which)
    assert math.isnan(loss)
    assert not any(g.any() for g in grads.values())              # the NaN loss sends NaN to every parameter
    # the running statistics say where it entered: layers 0..2 clean, channel 5 of layer 3, every channel behind it
    for n in ("conv.1", "conv.4", "conv.7"):
        assert bufs[n + ".running_mean"].all() and bufs[n + ".running_var"].all()
    only = torch.arange(N.C) != N.STEP_POISON[1][0]
    assert torch.equal(bufs["conv.10.running_mean"], only) and torch.equal(bufs["conv.10.running_var"], only)
    for n in ("conv.13", "conv.16", "conv.19"):
        assert not bufs[n + ".running_mean"].any() and not bufs[n + ".running_var"].any()


def test_reinforce_names_the_tensor_the_engine_refused():
    """LeafEngine.set_weights raises ValueError for BK_ERR_ARG; after an update REINFORCE turns the refusal of weights that
    are not finite into the FloatingPointError its other non-finite stops raise, and leaves every other refusal alone."""
    from bokego_amd import reinforce

    class Engine:
        def __init__(self, message):
            self.message = message

        def set_weights(self, sd):
            raise ValueError(self.message)

    net = torch.nn.Linear(1, 1)
    with pytest.raises(FloatingPointError, match=r"iteration 3: .*policy conv\.6\.weight"):
        reinforce._set_weights(Engine("BK_ERR_ARG: weights are not finite: policy conv.6.weight"), net, 3)
    with pytest.raises(ValueError, match="tickets outstanding"):
        reinforce._set_weights(Engine("BK_ERR_ARG: tickets outstanding"), net, 3)

