"""CPU: the one record of the playout options (bokego_amd/playout_options.py) -- every rule refused on the three
command lines with the flag named, the keywords and the engine name it builds, and the same rules from keywords."""
import pytest

from bokego_amd import gtp, match, selfplay
from bokego_amd.mcts_native import NativeMCTS, Position
from bokego_amd.playout_options import PlayoutOptions

V, VP = ["--playout-value", "8"], ["--playout-value", "8", "--playout-prior", "1"]
# (what parses, what is refused when added to it, the flag the message names)
SHARED = [
    ([], ["--playout-value", "-1"], "--playout-value"),
    ([], ["--playout-patterns", "p.npy"], "--playout-patterns"),
    ([], ["--playout-tactics", "t.npy"], "--playout-tactics"),
    ([], ["--playout-prior", "0.5"], "--playout-prior"),
    (V, ["--playout-prior", "1.5"], "--playout-prior"),
    (V, ["--playout-prior", "-0.5"], "--playout-prior"),
    (VP, ["--playout-criticality", "-1"], "--playout-criticality"),
    (VP, ["--playout-criticality", "nan"], "--playout-criticality"),
    (VP + ["--playout-patterns", "p.npy"], ["--playout-pattern-prior", "inf"], "--playout-pattern-prior"),
    (VP + ["--playout-patterns", "p.npy"], ["--playout-pattern-prior", "-2"], "--playout-pattern-prior"),
    (V, ["--playout-criticality", "0.5"], "--playout-criticality"),
    (V + ["--playout-tactics", "t.npy"], ["--playout-pattern-prior", "1"], "--playout-pattern-prior"),
    (VP, ["--playout-pattern-prior", "1"], "--playout-pattern-prior"),                  # no table at all
    (VP, ["--prior-patterns", "p.npy"], "--prior-patterns"),                            # a table without its term
    (VP, ["--prior-tactics", "t.npy"], "--prior-tactics"),
]
RAVE = [
    ([], ["--playout-rave"], "--playout-rave"),
    (V, ["--playout-rave", "-1"], "--playout-rave"),
    (V, ["--playout-rave", "inf"], "--playout-rave"),
]
OWN = {
    gtp: RAVE + [(V, ["-v", "v.pt"], "-v"), (V, ["--simulate"], "--simulate"), (V, ["--python-tree"], "--python-tree")],
    match: RAVE + [(V, ["--engine", "python -m oracle.gtp_cpu"], "--engine")],
    selfplay: [(V, ["--value", "v.pt"], "--value"), (V, ["--host-encode"], "--host-encode"), (VP, ["--policy", "p.pt"], "--policy")],
}


@pytest.mark.parametrize("mod", [gtp, match, selfplay], ids=lambda m: m.__name__.split(".")[-1])
def test_every_rule_is_refused_with_the_flag_named(mod, capsys):
    for good, added, flag in SHARED + OWN[mod]:
        assert isinstance(mod.parse_args(good).playout, PlayoutOptions), good
        with pytest.raises(SystemExit) as stop:
            mod.parse_args(good + added)
        assert stop.value.code == 2, good + added
        err = capsys.readouterr().err
        assert flag in err.splitlines()[-1].split("error:", 1)[1], (good + added, err)
    assert not hasattr(selfplay.parse_args([]), "playout_rave")
    assert mod.parse_args(VP + ["--prior-tactics", "t.npy", "--playout-pattern-prior", "0.5"]).prior_tactics == "t.npy"
    if mod is not selfplay:
        assert mod.parse_args(V + ["--playout-rave"]).playout_rave == 4.0 and mod.parse_args(V).playout_rave == 0.0


LINES = [   # (command line, NativeMCTS's keywords, match's name after boke-hip-r400, PlayoutEvaluator's keywords less the three below)
    (["--playout-value", "64"], dict(playout_value=64), "-mc64", {}),
    (["--playout-value", "32", "--playout-patterns", "p.npy"], dict(playout_value=32, playout_patterns="p.npy"), "-mc32-pat",
     dict(patterns="p.npy")),
    (["--playout-value", "32", "--playout-tactics", "t.npy", "--playout-prior", "0.5"],
     dict(playout_value=32, playout_tactics="t.npy", playout_prior=0.5), "-mc32-pat-amaf0.5", dict(tactics="t.npy", prior=0.5)),
    (["--playout-value", "64", "--playout-prior", "1", "--playout-rave"], dict(playout_value=64, playout_prior=1.0, playout_rave=4.0),
     "-mc64-amaf1-rave4", dict(prior=1.0, rave=True)),
    (["--playout-value", "64", "--playout-prior", "1", "--playout-rave", "16", "--playout-criticality", "0.25"],
     dict(playout_value=64, playout_prior=1.0, playout_rave=16.0, playout_criticality=0.25), "-mc64-amaf1-rave16-crit0.25",
     dict(prior=1.0, rave=True, criticality=0.25)),
    (["--playout-value", "64", "--playout-prior", "1", "--playout-pattern-prior", "1.5", "--playout-patterns", "p.npy",
      "--prior-tactics", "b.npy"],
     dict(playout_value=64, playout_prior=1.0, playout_patterns="p.npy", playout_pattern_prior=1.5, prior_patterns=None,
          prior_tactics="b.npy"), "-mc64-pat-amaf1-pp1.5",
     dict(prior=1.0, patterns="p.npy", pattern_prior=1.5, prior_patterns=None, prior_tactics="b.npy")),
]


def test_the_keywords_and_the_name_of_six_command_lines():
    assert {k for _, kw, _, _ in LINES for k in kw} == set(vars(PlayoutOptions())) - {"playout_seed", "playout_rules"}
    for argv, search, name, evaluator in LINES:
        for mod in (gtp, match) + (() if "--playout-rave" in argv else (selfplay,)):
            opts = mod.parse_args(argv).playout
            assert opts.search_keywords() == search, (mod, argv)
            assert opts.name_suffix() == name
            assert opts.evaluator_keywords() == dict(playouts=search["playout_value"], seed=0, rules="device", **evaluator)
    assert match.parse_args([]).playout.search_keywords() == {}


KEYWORDS = [
    (dict(playout_value=-1), ValueError, "playout_value"),
    (dict(playout_patterns="p.npy"), TypeError, "playout_value"),
    (dict(playout_tactics="t.npy"), TypeError, "playout_value"),
    (dict(playout_prior=0.5), TypeError, "playout_value"),
    (dict(playout_rave=4.0), TypeError, "playout_value"),
    (dict(playout_value=2, playout_prior=1.5), ValueError, "playout_prior"),
    (dict(playout_value=2, playout_rave=-1.0), ValueError, "playout_rave"),
    (dict(playout_value=2, playout_prior=1.0, playout_criticality=float("nan")), ValueError, "playout_criticality"),
    (dict(playout_value=2, playout_prior=1.0, playout_pattern_prior=float("inf"), prior_patterns="p.npy"), ValueError,
     "playout_pattern_prior"),
    (dict(playout_value=2, playout_criticality=0.5), TypeError, "playout_prior"),
    (dict(playout_value=2, playout_pattern_prior=1.0, prior_patterns="p.npy"), TypeError, "playout_prior"),
    (dict(playout_value=2, prior_patterns="p.npy"), TypeError, "playout_prior"),
    (dict(playout_value=2, prior_tactics="t.npy"), TypeError, "playout_prior"),
    (dict(playout_value=2, playout_prior=1.0, playout_pattern_prior=1.0), ValueError, "table"),
]


def test_the_same_rules_from_keywords():
    for kw, kind, names in KEYWORDS:
        with pytest.raises(kind, match=names):
            PlayoutOptions.from_keywords(kw)
        with pytest.raises(kind, match=names):
            NativeMCTS(Position(), None, None, playout_rules="host", **kw)
    # the one difference: a table of the pattern term may stay in place while the term is off -- not so on a command line
    kept = PlayoutOptions.from_keywords(dict(playout_value=2, playout_prior=1, prior_patterns="p.npy", playout_seed=3, playout_rules="host"))
    assert kept == PlayoutOptions(2, 3, "host", playout_prior=1.0, prior_patterns="p.npy")
    assert kept.search_keywords() == dict(playout_value=2, playout_prior=1.0)
    assert kept.evaluator_keywords() == dict(playouts=2, seed=3, rules="host", prior=1.0)
    assert PlayoutOptions.from_keywords({}) == PlayoutOptions() and PlayoutOptions.from_keywords(dict(playout_value=None)) == PlayoutOptions()
