""".multimerge on the device (HipContext.read_peaks(text_keys=True) / merge_peaks and the pipeline mirrors with device_merge=True) against
the plain-Python twin of the rule above chicdiff_hip_peaks_textkeys_dev in include/chicdiff_hip.h (tests/peaks_merge_twin.py;
tests/test_peaks_merge.py holds the twin to the host reader).  Everything is compared exactly: keys and hashes as int64, int32 columns
equal, fp64 columns as int64 bit patterns (NaN included), orders, source rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peaks_merge_inputs as mi  # noqa: E402
import peaks_merge_twin as mt  # noqa: E402
import peaks_twin as tw  # noqa: E402
from test_peaks_merge import CASES, bits, decline_cases, key_corpus, same_keys, token_file, word_files  # noqa: E402

gpu = pytest.mark.gpu
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 20011]
FALLBACK = "reading the peak matrix on the host"


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def device_keys(pk):
    return dict(status=pk.key_status, key_class=tuple(pk.key_class), chr_keys=pk.chr_keys.cpu().numpy(), name_hash=pk.name_hash.cpu().numpy())


def check_keys(ctx, path, note, targets=()):
    pk = ctx.read_peaks(path, list(targets), text_keys=True)
    assert pk.status == 0 and pk.chr_keys.shape == (2, pk.n) and pk.name_hash.shape == (2, pk.n), note
    return same_keys(device_keys(pk), path, note), pk


# ---- 1. text keys ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nrows", ROWS)
def test_text_keys_equal_the_twin_at_every_size(ctx, tmp_path, nrows):
    for chrom in ("text", "int"):
        (path,), _, _ = mi.make_set(tmp_path, 200 + nrows, [nrows], "none", chrom, tag=chrom)
        t, pk = check_keys(ctx, path, (nrows, chrom))
        assert pk.n == nrows and (nrows == 0 or t["key_class"] == ((mt.KEY_TEXT,) * 2 if chrom == "text" else (mt.KEY_INT,) * 2))


@gpu
def test_text_keys_other_separators_crlf_and_every_class(ctx, tmp_path):
    for k, kw in enumerate([dict(sep=","), dict(sep=" "), dict(crlf=True), dict(sep=",", crlf=True)]):
        (path,), _, _ = mi.make_set(tmp_path, 300 + k, [300], "none", "text", tag=f"v{k}", **kw)
        check_keys(ctx, path, kw)
    seen = set()
    for path, note in key_corpus(tmp_path):
        t, _ = check_keys(ctx, path, note)
        seen.add(t["key_class"])
    assert seen >= {(mt.KEY_TEXT, mt.KEY_TEXT), (mt.KEY_INT, mt.KEY_INT), (mt.KEY_MIXED, mt.KEY_MIXED), (mt.KEY_INT, mt.KEY_TEXT)}


@gpu
def test_text_keys_a_name_longer_than_a_tile(ctx, tmp_path):
    from chicdiff_amd import hip
    T = hip.peaks_caps()["tile_bytes"]
    for field in ("baitName", "oeName"):
        for at in (0, 20, 39):
            rows = [mi.base_row(oeID=9 + k, **({field: "g" * (T + 77 + k)} if k == at else {})) for k in range(40)]
            path = str(tmp_path / f"long_{field}_{at}.txt")
            mi.write_file(path, ["A0", "B0"], rows)
            t, pk = check_keys(ctx, path, (field, at))
            assert len(set(t["name_hash"][field == "oeName"])) == 2


BAD = [("chr1_random", mt.ST_CHR_LONG), ("1.0", mt.ST_CHR_AMBIGUOUS), ("NA", mt.ST_CHR_AMBIGUOUS), ("inf", mt.ST_CHR_AMBIGUOUS), ("01", mt.ST_CHR_AMBIGUOUS),
       ("café", mt.ST_CHR_AMBIGUOUS), ("1234567890", mt.ST_CHR_AMBIGUOUS), ("+infinity", mt.ST_CHR_LONG)]


@gpu
@pytest.mark.parametrize("tok,bit", BAD, ids=[repr(t) for t, _ in BAD])
def test_text_keys_every_status_case_in_the_first_a_middle_and_the_last_row(ctx, tmp_path, tok, bit):
    n = 300
    for at in (0, n // 2, n - 1):
        for column in (0, 1):
            toks = [["chr1"] * n, ["chr1"] * n]
            toks[column][at] = tok
            path = token_file(tmp_path, f"st_{at}_{column}.txt", toks[0], toks[1])
            t, pk = check_keys(ctx, path, (tok, at, column))
            assert pk.key_status == bit
    # a 9-digit number among strings: LONG; among numbers: a plain integer
    path = token_file(tmp_path, "nine.txt", ["123456789"] + ["chrX"] * 70, ["chrX"] * 71)
    assert check_keys(ctx, path, "nine among strings")[1].key_status == mt.ST_CHR_LONG
    path = token_file(tmp_path, "nine_int.txt", ["123456789"] + ["7"] * 70, ["3"] * 71)
    t, pk = check_keys(ctx, path, "nine among numbers")
    assert pk.key_status == 0 and pk.key_class == (mt.KEY_INT, mt.KEY_INT) and int(pk.chr_keys[0, 0]) == 123456789


@gpu
def test_read_peaks_without_the_keyword_is_what_it_was(ctx, tmp_path):
    (path,), chicago, targets = mi.make_set(tmp_path, 9, [3001], "none", "text")
    targets = [t for t in targets if t in mt.header_names(path)]
    t = tw.read_and_filter(path, targets, chicago, mi.SCORE)["all"]
    plain = ctx.read_peaks(path, targets)
    keyed = ctx.read_peaks(path, targets, text_keys=True)
    assert plain.chr_keys is None and plain.name_hash is None and plain.key_class is None and plain.key_status is None and plain.src_file is None
    for pk in (plain, keyed):
        assert pk.ints.dtype == ctx.torch.int32 and np.array_equal(pk.ints.cpu().numpy(), t["ints"])
        assert np.array_equal(bits(pk.dist.cpu().numpy()), bits(t["dist"])) and np.array_equal(bits(pk.scores.cpu().numpy()), bits(t["scores"]))
        assert np.array_equal(pk.line_off.cpu().numpy(), t["line_off"]) and pk.maxbait == int(t["ints"][2].max())
    assert plain.info == keyed.info and plain.score_names == keyed.score_names


@gpu
def test_text_keys_need_the_read_that_came_last(ctx, tmp_path):
    import ctypes as C
    from chicdiff_amd import hip
    (path,), _, _ = mi.make_set(tmp_path, 10, [50], "none", "text")
    ctx.read_peaks(path, [])
    with pytest.raises(hip.ChicdiffHipError, match="room for"):
        ctx._check(ctx.lib.chicdiff_hip_peaks_textkeys_dev(ctx.h, None, None, 10, (C.c_int64 * 4)()))
    with pytest.raises(hip.ChicdiffHipError):
        ctx.read_peaks(str(tmp_path / "missing.txt"), [])
    with pytest.raises(hip.ChicdiffHipError, match="holds no peak matrix"):
        ctx._check(ctx.lib.chicdiff_hip_peaks_textkeys_dev(ctx.h, None, None, 0, (C.c_int64 * 4)()))


# ---- 2. merged tables -----------------------------------------------------------------------------------------------------------------
def has_targets(paths, targets):
    return [[t for t in targets if t in mt.header_names(p)[11:]] for p in paths]


def device_merge(ctx, paths, targets):
    pks = [ctx.read_peaks(p, h, text_keys=True) for p, h in zip(paths, has_targets(paths, targets))]
    return ctx.merge_peaks(pks), pks


def check_merge(ctx, paths, targets, tag):
    files = [mt.read_file(p, h) for p, h in zip(paths, has_targets(paths, targets))]
    m = mt.merge(files)
    got, pks = device_merge(ctx, paths, targets)
    assert m["status"] == 0 and got.status == 0 and got.n == m["n_out"], (tag, got.status, got.n)
    assert got.ints.dtype == ctx.torch.int32 and np.array_equal(got.ints.cpu().numpy(), m["ints"]), tag
    assert np.array_equal(bits(got.dist.cpu().numpy()), bits(m["dist"])), tag
    assert got.scores.shape == m["scores"].shape and np.array_equal(bits(got.scores.cpu().numpy()), bits(m["scores"])), tag
    assert np.array_equal(got.src_file.cpu().numpy(), m["src_file"]) and np.array_equal(got.src_row.cpu().numpy(), m["src_row"]), tag
    want_off = np.array([files[f]["line_off"][r] for f, r in zip(m["src_file"], m["src_row"])], dtype=np.int64)
    assert np.array_equal(got.line_off.cpu().numpy(), want_off), tag
    assert got.score_names == [c for d in files for c in d["names"]] and got.paths == list(paths), tag
    assert got.maxbait == max([int(d["ints"][2].max()) for d in files if d["n"]], default=-1), tag
    return m, got


@gpu
@pytest.mark.parametrize("overlap", ["none", "all", "half"])
@pytest.mark.parametrize("nrows", ROWS)
@pytest.mark.parametrize("F", [2, 3, 4])
def test_merge_equals_the_twin(ctx, tmp_path, F, nrows, overlap):
    chrom = "text" if (F + nrows) % 2 else "int"
    paths, _, targets = mi.make_set(tmp_path, 1000 + 10 * nrows + F, [nrows] * F, overlap, chrom)
    m, _ = check_merge(ctx, paths, targets, (F, nrows, overlap))
    if overlap == "all":
        assert m["n_out"] == nrows
    if overlap == "none":
        assert m["n_out"] == F * nrows


@gpu
@pytest.mark.parametrize("nrows", [[1, 20011], [20011, 1], [257, 1, 1025], [0, 300], [65, 0, 64, 1]], ids=str)
def test_merge_files_of_unequal_length(ctx, tmp_path, nrows):
    paths, _, targets = mi.make_set(tmp_path, 31, nrows, "half", "text")
    check_merge(ctx, paths, targets, nrows)


@gpu
def test_merge_sorts_on_every_one_of_the_eight_words(ctx, tmp_path):
    paths, _, targets, rows = word_files(tmp_path)
    m, got = check_merge(ctx, paths, targets, "words")
    assert m["n_out"] == len(rows)
    # the order is the twin's: no two neighbours out of order in the words the twin sorts on
    f = [mt.read_file(p, h) for p, h in zip(paths, has_targets(paths, targets))]
    key = lambda k: (f[m["src_file"][k]]["chr_keys"][0][m["src_row"][k]],) + tuple(int(v) for v in m["ints"][:3, k]) + \
        (f[m["src_file"][k]]["chr_keys"][1][m["src_row"][k]],) + tuple(int(v) for v in m["ints"][3:, k])
    assert all(key(k) < key(k + 1) for k in range(m["n_out"] - 1))


@gpu
@pytest.mark.parametrize("F", [2, 3, 4])
def test_merge_a_group_of_every_file_across_positions_255_256_and_1023_1024(ctx, tmp_path, F):
    """Keys differ in oeID alone, so the sorted position of a row is known: 255 rows of one file each, the first shared key at sorted
    positions 255 .. 255 + F - 1, rows of one file each up to position 1022, the second shared key from 1023 on, a tail."""
    first, second = 255, 1023 - F + 1                                            # the shared keys' oeIDs = their ranks among the keys
    rows = [[] for _ in range(F)]
    rng = np.random.default_rng(F)
    for oe in range(second + 40):
        r = mi.base_row(oeID=oe, oeName=f"o{oe}", scores=("%d.5" % (oe % 9), "7.25"))
        for f in (range(F) if oe in (first, second) else [oe % F]):
            rows[f].append(r)
    paths = []
    chicago, targets, names = mi.design(F)
    for f in range(F):
        rng.shuffle(rows[f])
        paths.append(str(tmp_path / f"g{f}.txt"))
        mi.write_file(paths[f], names[f], rows[f])
    m, got = check_merge(ctx, paths, targets, F)
    assert m["n_out"] == second + 40
    for key in (first, second):
        assert int(m["ints"][5][key]) == key and not np.isnan(m["scores"][:, key]).any()      # every file's cells
        assert np.isnan(m["scores"][:, key - 1]).sum() == 2 * (F - 1)
    at2 = second + F - 1                                                         # sorted position of the second group's first row
    assert first <= 255 < 256 <= first + F - 1 and at2 <= 1023 < 1024 <= at2 + F - 1


def permuted_copy(path, out, seed):
    data = open(path, "rb").read()
    nl = data.index(b"\n") + 1
    lines = data[nl:].splitlines(keepends=True)
    np.random.default_rng(seed).shuffle(lines)
    open(out, "wb").write(data[:nl] + b"".join(lines))
    return out


@gpu
def test_merge_does_not_depend_on_input_order_and_repeats_bit_for_bit(ctx, tmp_path):
    paths, _, targets = mi.make_set(tmp_path, 55, [1500, 1200, 900], "half", "text", shuffle=False)
    m, a = check_merge(ctx, paths, targets, "as written")
    other = [permuted_copy(p, str(tmp_path / f"perm{k}.txt"), k) for k, p in enumerate(paths)]
    m2, b = check_merge(ctx, other, targets, "rows permuted")
    again, _ = device_merge(ctx, paths, targets)
    for x in (b, again):
        assert np.array_equal(a.ints.cpu().numpy(), x.ints.cpu().numpy()) and np.array_equal(bits(a.dist.cpu().numpy()), bits(x.dist.cpu().numpy()))
        assert np.array_equal(bits(a.scores.cpu().numpy()), bits(x.scores.cpu().numpy())) and np.array_equal(a.src_file.cpu().numpy(), x.src_file.cpu().numpy())
    assert np.array_equal(a.src_row.cpu().numpy(), again.src_row.cpu().numpy()) and np.array_equal(a.line_off.cpu().numpy(), again.line_off.cpu().numpy())
    assert not np.array_equal(a.src_row.cpu().numpy(), b.src_row.cpu().numpy())


# ---- 3. declined merges ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", CASES)
def test_declined_merges_give_their_status_bit_one_message_and_the_host_result(ctx, tmp_path, capsys, name):
    from chicdiff_amd import hip, pipeline
    paths, targets, chicago, why = decline_cases(tmp_path)[name]
    if name != "target_in_two_files":
        pks = [ctx.read_peaks(p, h, text_keys=True) for p, h in zip(paths, has_targets(paths, targets))]
        key_status = 0
        for pk in pks:
            key_status |= pk.key_status
        want_key = {"long_chr": hip.PEAKS_ST_CHR_LONG, "ambiguous_chr": hip.PEAKS_ST_CHR_AMBIGUOUS, "na_chr": hip.PEAKS_ST_CHR_AMBIGUOUS}.get(name, 0)
        assert key_status == want_key, name
        want_merge = {"duplicate_key": hip.PEAKS_ST_MERGE_DUPLICATE, "bait_name": hip.PEAKS_ST_MERGE_NAME, "oe_name": hip.PEAKS_ST_MERGE_NAME,
                      "dist": hip.PEAKS_ST_MERGE_DIST, "dist_na": hip.PEAKS_ST_MERGE_DIST}.get(name)
        if want_merge:
            m = ctx.merge_peaks(pks)
            assert m.status & want_merge and m.ints is None, (name, m.status)
            assert name == "duplicate_key" or m.status == want_merge, (name, m.status)
        if name == "int_against_text":
            assert pks[0].key_class == (hip.PEAKS_KEY_INT, hip.PEAKS_KEY_INT) and pks[1].key_class == (hip.PEAKS_KEY_TEXT, hip.PEAKS_KEY_TEXT)
        if name == "header_only":
            assert pks[1].n == 0 and pks[1].status == 0
    args = (paths, targets, chicago, list(chicago), mi.SCORE)
    capsys.readouterr()
    if mt.decline(paths, targets)[1] == "raise":
        with pytest.raises(ValueError):
            pipeline.readAndFilterPeakMatrix(*args, outprefix=str(tmp_path / "h"))
        with pytest.raises(ValueError):
            pipeline.readAndFilterPeakMatrix(*args, outprefix=str(tmp_path / "d"), ctx=ctx, device=True, device_merge=True)
        assert capsys.readouterr().err.count(FALLBACK) == 1
        return
    want = pipeline.readAndFilterPeakMatrix(*args, outprefix=str(tmp_path / "h"))
    pm = pipeline.readAndFilterPeakMatrix(*args, outprefix=str(tmp_path / "d"), ctx=ctx, device=True, device_merge=True)
    assert capsys.readouterr().err.count(FALLBACK) == 1
    got = pm.to_frame()
    assert got is pm.frame and list(got.columns) == list(want.columns) and len(got) == len(want)
    for c in want.columns:
        assert got[c].astype(str).tolist() == want[c].astype(str).tolist(), c
    assert open(str(tmp_path / "h") + "_filteredBaits.txt", "rb").read() == open(str(tmp_path / "d") + "_filteredBaits.txt", "rb").read()


@gpu
def test_a_target_that_no_file_holds_raises_the_reference_message_on_the_device_path(ctx, tmp_path):
    from chicdiff_amd import pipeline
    paths, chicago, targets = mi.make_set(tmp_path, 3, [40, 40], "half", "text")
    with pytest.raises(ValueError, match="All specified targetColumns must be present in the peak file"):
        pipeline.readAndFilterPeakMatrix(paths, targets + ["nowhere"], chicago, list(chicago), mi.SCORE, outprefix=str(tmp_path / "d"), ctx=ctx,
                                         device=True, device_merge=True)


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nrows,chrom,per_file", [([5000, 4500], "text", 2), ([5000, 4000, 4500], "int", 2), ([5000, 5000], "text", 1)],
                         ids=["2-files-text", "3-files-int", "2-files-no-replicate-rule"])
def test_mirror_read_merge_and_filter_against_the_host_path(ctx, tmp_path, capsys, monkeypatch, nrows, chrom, per_file):
    import pandas as pd
    from chicdiff_amd import pipeline
    paths, chicago, targets = mi.make_set(tmp_path, 70 + len(nrows), nrows, "half", chrom, per_file=per_file)
    args = (paths, targets, chicago, list(chicago), mi.SCORE)
    want = pipeline.readAndFilterPeakMatrix(*args, outprefix=str(tmp_path / "h"))
    capsys.readouterr()
    with monkeypatch.context() as mp:                                             # no host read of a peak file on the device path
        mp.setattr(pd, "read_csv", lambda *a, **k: pytest.fail("the host reader ran"))
        pm = pipeline.readAndFilterPeakMatrix(*args, outprefix=str(tmp_path / "d"), ctx=ctx, device=True, device_merge=True)
        got = pm.to_frame()
    assert FALLBACK not in capsys.readouterr().err and pm.frame is None
    assert open(str(tmp_path / "h") + "_filteredBaits.txt", "rb").read() == open(str(tmp_path / "d") + "_filteredBaits.txt", "rb").read()
    assert list(got.columns) == list(want.columns) and len(got) == len(want) > 100
    assert np.array_equal(pm["baitID"].cpu().numpy(), want["baitID"].to_numpy(np.int32)) and np.array_equal(pm["oeID"].cpu().numpy(), want["oeID"].to_numpy(np.int32))
    for c in want.columns:
        if c in ("baitChr", "baitName", "oeChr", "oeName"):
            assert got[c].tolist() == want[c].astype(str).tolist(), c                # documented: text columns are strings
        elif want[c].dtype == np.float64:
            assert np.array_equal(bits(got[c].to_numpy()), bits(want[c].to_numpy())), c   # 6-digit tokens: both readers give float(token)
        else:
            assert np.array_equal(got[c].to_numpy(np.int64), want[c].to_numpy(np.int64)), c
    t = mt.read_and_filter(paths, targets, chicago, mi.SCORE)
    assert np.array_equal(pm["src_file"].cpu().numpy(), t["merged"]["src_file"][t["kept"]])
    # without the keyword: the present message and the host reader
    pm2 = pipeline.readAndFilterPeakMatrix(*args, outprefix=str(tmp_path / "e"), ctx=ctx, device=True)
    assert "more than one peak file (.multimerge stays host code)" in capsys.readouterr().err and pm2.frame is not None and len(pm2.frame) == len(want)


@pytest.fixture(scope="module")
def split_experiment(tmp_path_factory):
    """The experiment of tests/pipeline_inputs.py with its peak matrix split in two: the first half of the score columns for every row,
    the second half for four rows in five, in another order."""
    from pipeline_inputs import make_experiment
    tmp = tmp_path_factory.mktemp("peaks_merge_experiment")
    settings, truth = make_experiment(tmp, npeaks=2500)
    lines = open(settings["peakfiles"][0]).read().splitlines()
    header, body = lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]
    T = len(header) - 11
    a, b = str(tmp / "peaks_a.txt"), str(tmp / "peaks_b.txt")
    with open(a, "w") as f:
        f.write("\n".join("\t".join(r[:11 + T // 2]) for r in [header] + body) + "\n")
    rng = np.random.default_rng(1)
    some = [body[k] for k in rng.permutation(len(body))[: 4 * len(body) // 5]]
    with open(b, "w") as f:
        f.write("\n".join("\t".join(r[:11] + r[11 + T // 2:]) for r in [header] + some) + "\n")
    settings = dict(settings)
    settings["peakfiles"] = [a, b]
    return settings


@gpu
def test_mirror_region_universe_from_merged_device_peaks(ctx, split_experiment, capsys):
    import inspect
    from chicdiff_amd import pipeline
    want = pipeline.getRegionUniverse(split_experiment, ctx)
    capsys.readouterr()
    got = pipeline.getRegionUniverse(split_experiment, ctx, device_peaks=True, device_merge=True)
    assert FALLBACK not in capsys.readouterr().err
    assert set(got) == set(want) and want["region_ptr"].numel() > 100
    for k in want:
        x, y = got[k], want[k]
        x, y = (x.cpu().numpy(), y.cpu().numpy()) if hasattr(x, "cpu") else (np.asarray(x), np.asarray(y))
        assert x.dtype == y.dtype and np.array_equal(x, y), k
    for fn in (pipeline.readAndFilterPeakMatrix, pipeline.getRegionUniverse, pipeline.chicdiffPipeline):
        assert inspect.signature(fn).parameters["device_merge"].default is False
