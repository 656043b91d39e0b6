"""The random-missing protocol on the host (sdumc_amd/data.py: MissingSpec, missing_keep; DeviceFeatureStore.with_missing's validation).
Every expectation is the rule of include/sdumc_hip.h evaluated HERE with oracle/philox.py's Philox4x32-10:

  word(c0) = philox4x32_10(c0, utt, 0x4D530000 + m, draw, seed & 0xffffffff, seed >> 32)[0]
  frame t of modality m of utterance utt is absent  iff  word(t) < floor(frame[m] * 2^32)  or  word(0xFFFFFFFF) < floor(modality[m] * 2^32)

with oracle.philox.drop_threshold's comparison; a rate of 1 makes every frame absent (its threshold is 2^32: compared in Python ints)."""
import numpy as np
import pytest

from oracle.philox import philox4x32_10, drop_threshold

MODS = ("audio", "text", "video", "feat4")


def rule_absent(frame, modality, seed, draw, m, utt, length):
    """bool [length], True = absent: the rule, from the oracle's Philox and Python integers (nothing of sdumc_amd)"""
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    t = np.arange(length, dtype=np.uint32)
    w_t = philox4x32_10(t, np.uint32(utt), np.uint32(0x4D530000 + m), np.uint32(draw), k0, k1)[0].astype(np.uint64)
    w_u = int(philox4x32_10(np.uint32(0xFFFFFFFF), np.uint32(utt), np.uint32(0x4D530000 + m), np.uint32(draw), k0, k1)[0])
    absent = w_t < np.uint64(drop_threshold(frame))      # (a threshold of 2^32 fits uint64: every word is below it)
    return absent | (w_u < drop_threshold(modality))


CASES = [  # (seed, draw, m, utt, length)
    (0, 0, 0, 0, 17), (1234, 3, 2, 36, 40), ((7 << 32) | 5, 1, 1, 5, 6), (2 ** 64 - 1, 2 ** 32 - 1, 3, 2 ** 31 + 7, 9),
    (2 ** 32, 2 ** 32 - 1, 0, 11, 1), (99, 7, 3, 123456, 1), (1234, 0, 1, 0, 64),
]


@pytest.mark.parametrize("seed,draw,m,utt,length", CASES)
def test_missing_keep_is_the_rule(seed, draw, m, utt, length):
    from sdumc_amd import data
    for fr, mr in ((0.3, 0.0), (0.0, 0.4), (0.5, 0.25), (0.9, 0.9)):
        spec = data.MissingSpec(frame={MODS[m]: fr}, modality={MODS[m]: mr}, seed=seed, draw=draw)
        want = ~rule_absent(fr, mr, seed, draw, m, utt, length)
        for name in (MODS[m], m):      # by name and by index
            got = data.missing_keep(spec, name, utt, length)
            assert got.dtype == np.bool_ and got.shape == (length,)
            np.testing.assert_array_equal(got, want)
        # a mapping with the spec's fields is accepted as well
        np.testing.assert_array_equal(data.missing_keep({"frame": {MODS[m]: fr}, "modality": {MODS[m]: mr}, "seed": seed, "draw": draw},
                                                        m, utt, length), want)
        # another modality of the same spec has rate 0: everything kept
        assert data.missing_keep(spec, (m + 1) % 4, utt, length).all()


def test_streams_differ_by_modality_draw_seed_and_utterance():
    """the counter carries the modality, the draw and the utterance; the key the seed: each changes the mask (64 frames at rate 0.5: two
    independent masks agree with probability 2^-64)"""
    from sdumc_amd import data
    def keep(m=0, utt=3, seed=1234, draw=0):
        return data.missing_keep(data.MissingSpec(frame={k: 0.5 for k in MODS}, seed=seed, draw=draw), m, utt, 64)
    base = keep()
    np.testing.assert_array_equal(base, keep())
    for other in (keep(m=1), keep(m=3), keep(utt=4), keep(seed=1235), keep(seed=1234 + 2 ** 32), keep(draw=1)):
        assert not np.array_equal(base, other)


def test_rate_zero_keeps_all_rate_one_keeps_none_and_the_levels_combine_by_or():
    from sdumc_amd import data
    for seed, draw, m, utt, length in CASES:
        name = MODS[m]
        assert data.missing_keep(data.MissingSpec(seed=seed, draw=draw), m, utt, length).all()
        assert data.missing_keep(data.MissingSpec(frame={name: 0.0}, modality={name: 0}, seed=seed, draw=draw), m, utt, length).all()
        assert not data.missing_keep(data.MissingSpec(frame={name: 1.0}, seed=seed, draw=draw), m, utt, length).any()
        assert not data.missing_keep(data.MissingSpec(modality={name: 1}, seed=seed, draw=draw), m, utt, length).any()
        assert not data.missing_keep(data.MissingSpec(frame={name: 0.1}, modality={name: 1.0}, seed=seed, draw=draw), m, utt, length).any()
    # OR: keep(frame and modality level) = keep(frame level alone) & keep(modality level alone); the modality level is all or nothing
    both_kinds = set()
    for utt in range(40):
        f = data.missing_keep(data.MissingSpec(frame={"audio": 0.4}, seed=5, draw=2), "audio", utt, 30)
        u = data.missing_keep(data.MissingSpec(modality={"audio": 0.5}, seed=5, draw=2), "audio", utt, 30)
        fu = data.missing_keep(data.MissingSpec(frame={"audio": 0.4}, modality={"audio": 0.5}, seed=5, draw=2), "audio", utt, 30)
        assert u.all() or not u.any()
        both_kinds.add(bool(u.all()))
        np.testing.assert_array_equal(fu, f & u)
        np.testing.assert_array_equal(u, ~rule_absent(0.0, 0.5, 5, 2, 0, utt, 30))
    assert both_kinds == {True, False}      # (40 utterances at rate 0.5: both outcomes occur)


@pytest.mark.parametrize("rate", [0.2, 0.5, 0.9])
@pytest.mark.parametrize("draw", [0, 1, 2])
@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_absent_share_is_the_rate(rate, draw, m):
    """64 utterances x 64 frames, seed 1234: |absent share - rate| <= 4 sqrt(rate (1 - rate) / 4096) -- four standard deviations of a
    binomial share over 4096 independent draws.  (With the oracle's Philox the worst of the 36 cases is 2.36 sigma.)"""
    from sdumc_amd import data
    spec = data.MissingSpec(frame={MODS[m]: rate}, seed=1234, draw=draw)
    keep = np.stack([data.missing_keep(spec, m, utt, 64) for utt in range(64)])
    want = np.stack([~rule_absent(rate, 0.0, 1234, draw, m, utt, 64) for utt in range(64)])
    np.testing.assert_array_equal(keep, want)
    share = 1.0 - keep.mean()
    assert abs(share - rate) <= 4.0 * np.sqrt(rate * (1.0 - rate) / 4096), (share, rate)


def test_thresholds_are_the_drop_threshold_convention():
    from sdumc_amd import data
    spec = data.MissingSpec(frame={"audio": 0.3, "text": 1.0, "video": 0.0}, modality={"audio": 0.25, "feat4": 1}, seed=1)
    assert spec.thresholds(0) == (drop_threshold(0.3), drop_threshold(0.25), 0)
    assert spec.thresholds(1) == (0xFFFFFFFF, 0, 1)      # a rate of 1: the flag, the threshold clamped to 32 bits
    assert spec.thresholds(2) == (0, 0, 0)
    assert spec.thresholds(3) == (0, 0xFFFFFFFF, 2)
    assert spec.enabled and not data.MissingSpec(frame={"audio": 0.0}, seed=9, draw=4).enabled
    assert spec.with_draw(7).draw == 7 and spec.with_draw(7).frame == spec.frame and spec.with_draw(7).seed == 1


class _HostStore:
    """what with_missing's validation needs of a store, without a device: DeviceFeatureStore's own method on a bare object"""

    def __new__(cls):
        from sdumc_amd.data import DeviceFeatureStore
        return DeviceFeatureStore.__new__(DeviceFeatureStore)


@pytest.mark.parametrize("kw", [
    {"frame": {"audio": 1.5}}, {"frame": {"audio": -0.1}}, {"modality": {"video": 2}}, {"modality": {"text": float("nan")}},
    {"frame": {"audio": "0.2"}}, {"frame": {"sound": 0.2}}, {"modality": {"feat5": 0.2}}, {"frame": 0.2},
    {"seed": -1}, {"seed": 2 ** 64}, {"seed": 1.5}, {"draw": -1}, {"draw": 2 ** 32}, {"draw": 0.0},
])
def test_bad_specs_raise_on_the_host(kw):
    from sdumc_amd import data, _lib
    with pytest.raises((_lib.SdumcError, ValueError)):
        data.MissingSpec(**kw)
    with pytest.raises((_lib.SdumcError, ValueError)):
        _HostStore().with_missing(**kw)
    with pytest.raises((_lib.SdumcError, ValueError)):
        data.missing_keep(kw, "audio", 0, 4)


def test_views_share_replace_and_refuse_to_resample():
    """a view holds its base and its spec and nothing else; with_missing on a view REPLACES the spec; redrawn keeps it at another draw;
    resampled raises (pool first, then view)"""
    from sdumc_amd import data, _lib
    store = _HostStore()
    store.names, store.marker = ["a", "b"], object()
    v = store.with_missing(frame={"audio": 0.2}, modality={"text": 0.5}, seed=3, draw=1)
    assert v.base is store and v.spec == data.MissingSpec(frame={"audio": 0.2}, modality={"text": 0.5}, seed=3, draw=1)
    assert set(vars(v)) == {"base", "spec", "_miss"} and v.marker is store.marker and len(v) == 2 and isinstance(v, data.DeviceFeatureStore)
    w = v.with_missing(frame={"video": 0.7})
    assert w.base is store and w.spec == data.MissingSpec(frame={"video": 0.7})      # replaced: audio and text are back, seed 0
    r = v.redrawn(9)
    assert r.base is store and r.spec == v.spec.with_draw(9) and r.spec.draw == 9 and v.spec.draw == 1
    assert v._miss == ((3, 0, 1), tuple(v.spec.thresholds(k) for k in range(4)))
    assert store.with_missing()._miss is None and store.with_missing(frame={"audio": 0.0}, seed=5)._miss is None      # all rates 0
    with pytest.raises(_lib.SdumcError, match="pool first"):
        v.resampled(2)
    with pytest.raises((_lib.SdumcError, ValueError)):
        v.redrawn(2 ** 32)
    for bad in ("sound", 4, -1, None, True):
        with pytest.raises((_lib.SdumcError, ValueError)):
            data.missing_keep(v.spec, bad, 0, 4)
    for utt, length in ((-1, 4), (2 ** 32, 4), (0, -1), (0.5, 4)):
        with pytest.raises((_lib.SdumcError, ValueError)):
            data.missing_keep(v.spec, "audio", utt, length)
