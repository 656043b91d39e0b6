"""The case matrix of tests/backward_cases.py, without a GPU: (1) the matrix itself -- every case named once, every setting expressible
through ExecContext.set_option, every storage admitted by its shape's widths, the coverage the matrix promises; (2) the reference side
of every case, from the oracle alone: with the fp32 evaluation playing the device, grad_parity.tensor_errors passes at the case's bar
and the classes stay inside the helper's caps (at most MAX_BETWEEN tensors in between or the named ones, no-signal tensors and exact
zeros only where named).  The caps are conditions on the shapes: a shape that breaks them gets another seed or other lengths, the
caps stay.  Prints the worst reference-side e_ref of every reference."""
import pytest

from tests import backward_cases as BC
from tests import grad_parity as GP

REF_KEYS = sorted({BC.ref_key(c) for c in BC.CASES if BC.has_reference(c)})


def test_matrix_names_every_case_once_and_covers_what_it_promises():
    ids = [BC.case_id(c) for c in BC.CASES]
    assert len(ids) == len(set(ids))
    for c in BC.CASES:
        assert c.shape in BC.SHAPES and c.storage in BC.STORAGES and c.form in BC.FORMS and c.setting in BC.SETTINGS, c
    have = set(BC.CASES)
    # the default and the seven single-option settings at the three fold shapes and no-fold
    for shape in ("fold-av", "fold-av-ne", "fold-all", "no-fold"):
        for setting in BC.SINGLES:
            assert BC.Case(shape, "fp32", "net", setting) in have
    # the remaining settings at fold-av and no-fold
    for shape in ("fold-av", "no-fold"):
        for setting in ("bg0+conc0", "bg0+cl0"):
            assert BC.Case(shape, "fp32", "net", setting) in have
        for setting in ("default", "conc0", "bg0"):
            assert BC.Case(shape, "fp32", "phased", setting) in have
        assert BC.Case(shape, "fp32", "s1", "default") in have and BC.Case(shape, "fp32", "eval", "default") in have
        assert BC.Case(shape, "bf16op", "net", "default") in have
    # the remaining shapes under the default, conc0 and bg0
    for shape in set(BC.SHAPES) - {"fold-av", "fold-av-ne", "fold-all", "no-fold"}:
        for setting in ("default", "conc0", "bg0"):
            assert any(c.shape == shape and c.setting == setting for c in have), (shape, setting)
    assert {c.form for c in have if c.form.startswith("step")} == {"step", "step-freeze", "step-freeze-all"}
    assert {c.storage for c in have if c.form == "step"} == {"planes", "bf16s", "fp32"}


# what ExecContext.set_option documents for each option (its docstring: 'concurrency' 0 | 1, 'background_lane' 0 | 2 | 3, 'chain_cluster'
# 0 | 1, 'split' 0..15), written out here and nowhere else in the tests
SET_OPTION_VALUES = {"concurrency": (0, 1), "background_lane": (0, 2, 3), "chain_cluster": (0, 1), "split": tuple(range(16))}


def test_every_setting_is_expressible_through_the_public_surface():
    """a setting is exactly the options ExecContext.set_option knows by name (engine.ExecContext.OPTIONS: loading the module needs the
    built library, no GPU), each at a value its docstring lists; the aliases and one-lane partners name what the matrix says they name"""
    from sdumc_amd import engine
    assert set(SET_OPTION_VALUES) == set(engine.ExecContext.OPTIONS) == set(BC.DEFAULT)
    assert BC.OPTION_VALUES == SET_OPTION_VALUES
    assert len(BC.SINGLES) == 8 and set(BC.SINGLES) <= set(BC.SETTINGS)
    for name in list(BC.SETTINGS) + list(BC.ALIASES) + list(BC.ONE_LANE):
        opts = BC.options(name)
        assert set(opts) == set(engine.ExecContext.OPTIONS)
        for k, v in opts.items():
            assert v in SET_OPTION_VALUES[k], (name, k, v)
    for alias, same in BC.ALIASES.items():
        assert same in BC.SETTINGS and alias not in BC.SETTINGS
    assert BC.options("bg3+conc0") == BC.options("conc0") and BC.options("split7+bg3") == BC.options("split7")
    # the one-lane partner of a multi-lane setting differs from it in concurrency alone; partners that are no setting of the matrix stay
    # out of SETTINGS (the route table has no row for them)
    assert set(BC.ONE_LANE_PARTNERS) == {n for n in BC.SETTINGS if BC.options(n)["concurrency"] == 1}
    for n, p in BC.ONE_LANE_PARTNERS.items():
        assert BC.options(p) == {**BC.options(n), "concurrency": 0} and (p in BC.SETTINGS) != (p in BC.ONE_LANE)
    assert not {c.setting for c in BC.CASES} & set(BC.ONE_LANE)
    # one setting, one set of options: no two names run the same thing
    seen = {}
    for name in list(BC.SETTINGS) + list(BC.ONE_LANE):
        key = tuple(sorted(BC.options(name).items()))
        assert key not in seen, (name, seen.get(key))
        seen[key] = name


def test_every_storage_is_admitted_by_its_shape():
    """planes and bf16 storage need widths in whole 64-element tiles: elsewhere the Python surface silently takes another mode"""
    for c in BC.CASES:
        widths = BC.SHAPES[c.shape][0][:3]
        if c.storage in ("planes", "bf16s"):
            assert all(w % 64 == 0 for w in widths), c
        if c.form == "eval" and c.storage == "bf16s":
            assert c.shape == "bf16-few"


@pytest.mark.parametrize("key", REF_KEYS, ids=["%s-%s-%s" % (k[0], "emu" if k[1] else "fp32", k[2]) for k in REF_KEYS])
def test_reference_side_passes_and_stays_inside_the_caps(key):
    c = next(c for c in BC.CASES if BC.has_reference(c) and BC.ref_key(c) == key)
    ref = BC.reference(c)
    names = list(ref["hi"])
    assert len(names) == 83 and set(names) == set(ref["lo"])
    z = BC.zeros(c.shape, c.form)
    res = GP.tensor_errors(names, ref["lo"], ref["hi"], ref["lo"], BC.bar_of(c), zeros=z, what="%s, fp32 evaluation as the device" % (key,))
    assert sorted(res.zero) == sorted(z)
    if not c.form.startswith("step"):
        assert not res.nosignal      # O(1) external gradients: the RnC head's biases carry signal
    worst = max(res.e_ref, key=res.e_ref.get)
    print("backward routes %s: worst reference-side e_ref %s = %.3g" % (key, worst, res.e_ref[worst]))
    if "losses" in ref:
        assert all(v == v and abs(v) < float("inf") for v in ref["losses"])
