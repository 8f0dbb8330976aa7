"""countput on the host: the numpy twin written from the rule in include/chicdiff_hip.h (tests/countput_twin.py) equals the pandas
groupby of pipeline._countput (chicdiff.R:708-735, 754-768) bit for bit — every column, NaN in the same cells, the same row order —
and the inputs (tests/countput_inputs.py) can tell the rule from its neighbours: the plain left-to-right sum, and the Kahan sum
without the reset of a NaN compensation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import countput_inputs as cpi  # noqa: E402
from countput_twin import countput_twin  # noqa: E402

LENGTHS = {"one": (257,), "two": (300, 129), "three": (513, 420, 300), "four": (400, 1, 357, 290)}


def conditions_of(order, dups=False):
    """Four conditions of 1, 2, 3 and 4 replicates of different lengths over one map, as (frames, condition names, nid)."""
    xs, conds = [], []
    for seed, (name, lens) in enumerate(LENGTHS.items(), start=1):
        frames, nid = cpi.condition(lens, seed, order, dups)
        xs += frames
        conds += [name] * len(frames)
        assert nid == 400
    return xs, conds, 400


def twin_frame(xs, conds, nid, **kw):
    midsum, chr_codes, _ = cpi.the_map(nid)
    names = list(dict.fromkeys(conds))
    return cpi.frame_of([countput_twin([x for x, c in zip(xs, conds) if c == name], cpi.ID_MIN, midsum, chr_codes, **kw) for name in names], names)


@pytest.mark.parametrize("dups", [False, True], ids=["unique-pairs", "repeated-pairs"])
@pytest.mark.parametrize("order", cpi.ORDERS)
def test_twin_equals_the_pandas_groupby(order, dups):
    from chicdiff_amd import pipeline
    xs, conds, nid = conditions_of(order, dups)
    want = pipeline._countput(xs, conds, cpi.the_map(nid)[2])
    got = twin_frame(xs, conds, nid)
    cpi.assert_same_frame(got, want, (order, dups))
    # what the tables are meant to hold
    assert 0 < len(want) < sum(len(x) for x in xs)
    for k in ("Bav", "score"):
        assert want[k].isna().any() and want[k].notna().any(), k
    assert np.isinf(want["Bav"]).any()
    z = want["score"].to_numpy()
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    all_oe = np.concatenate([x["otherEndID"].to_numpy() for x in xs])
    all_bait = np.concatenate([x["baitID"].to_numpy() for x in xs])
    chr_codes = cpi.the_map(nid)[1]
    gap = cpi.ID_MIN + np.flatnonzero(chr_codes < 0)
    assert np.isin(all_oe, gap).any() and not np.isin(want["otherEndID"], gap).any()                 # the gap drops rows
    assert (all_oe < cpi.ID_MIN).any() and want["otherEndID"].min() >= cpi.ID_MIN                       # so do other ends off the map
    off = (want["baitID"] < cpi.ID_MIN) | (want["baitID"] >= cpi.ID_MIN + nid) | np.isin(want["baitID"], gap)
    assert off.any() and ((all_bait < cpi.ID_MIN) | (all_bait >= cpi.ID_MIN + nid)).any()            # baits off the map stay
    assert (want["oeID_mid"] % 1 == 0.5).any()


def test_hand_written_groups():
    """+-inf, inf - inf, signed zeros in both orders, a group without values, a pair repeated inside a replicate: the pandas groupby
    and the twin both give the values worked out by hand."""
    from chicdiff_amd import pipeline
    frames, nid = cpi.condition((300, 129, 65), 3)
    xs, expected = cpi.with_edges(list(frames), nid)
    conds = ["c"] * 3
    want = pipeline._countput(xs, conds, cpi.the_map(nid)[2])
    got = twin_frame(xs, conds, nid)
    cpi.assert_same_frame(got, want, "edges")
    for k, (nav, bav, score) in enumerate(expected):
        row = want[want["baitID"] == cpi.ID_MIN + nid + 100 + k]
        assert len(row) == 1, k
        for name, v in (("Nav", nav), ("Bav", bav), ("score", score)):
            assert cpi.same_bits(row[name].to_numpy(), [v]), (k, name, row[name].to_numpy(), v)
    assert want["baitID"].iloc[-1] == cpi.ID_MIN + nid + 105       # replicate 2's own pair: first seen in the table's last rows


def bits_differ(a, b):
    a, b = a.to_numpy(), b.to_numpy()
    return (np.isnan(a) != np.isnan(b)) | (~np.isnan(a) & ~np.isnan(b) & (a.view(np.int64) != b.view(np.int64)))


def test_inputs_tell_the_rule_from_its_neighbours():
    for name in ("three", "four"):
        frames, nid = cpi.condition(LENGTHS[name], list(LENGTHS).index(name) + 1)
        xs, conds = list(frames), [name] * len(frames)
        rule = twin_frame(xs, conds, nid)
        plain = twin_frame(xs, conds, nid, compensated=False)
        differs = bits_differ(rule["Bav"], plain["Bav"])
        assert differs.any(), name                                  # a plain sum in row order is not the rule
        assert cpi.same_bits(rule["Nav"].to_numpy(), plain["Nav"].to_numpy())    # (small integers: every sum is exact)
        noreset = twin_frame(xs, conds, nid, reset=False)
        changed = bits_differ(rule["Bav"], noreset["Bav"])
        assert changed.any(), name                                  # nor is a Kahan sum that keeps a NaN compensation
        assert np.isinf(rule["Bav"].to_numpy()[changed]).all() and np.isnan(noreset["Bav"].to_numpy()[changed]).all()


@pytest.mark.parametrize("scattered", [False, True], ids=["contiguous", "scattered"])
def test_one_pair_repeated_5000_times(scattered):
    """A group of thousands of rows: the twin's recurrence over the position in the group equals pandas' row loop."""
    from chicdiff_amd import pipeline
    frames, nid = cpi.repeated_pair(scattered)
    want = pipeline._countput(list(frames), ["c", "c"], cpi.the_map(nid)[2])
    cpi.assert_same_frame(twin_frame(list(frames), ["c", "c"], nid), want, scattered)
    big = want[(want["baitID"] == cpi.REP_BAIT) & (want["otherEndID"] == cpi.REP_OE)]
    assert len(big) == 1
