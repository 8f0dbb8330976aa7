"""Shared inputs of the control-draw tests: a restriction map of 1 100 fragments on four chromosomes, a baitmap of every 7th
fragment, and hand-picked peaks whose expansion (RUexpand = 5) gives each chromosome a known largest contact:

    IDs    1 ..  400   "10" (code 1)   largest contact 120      (140 -> 255: rows 250 .. 260)
    IDs  401 .. 1000   "2"  (code 2)   largest contact 590      (406 -> 991: rows 986 .. 996)
    IDs 1001 .. 1060   "X"  (code 3)   largest contact 2        (1058 -> 1059: rows 1060 .. 1064, the map ends the chromosome at 1060;
                                                                 a peak's bait comes from the peak matrix and need not be on the baitmap)
    IDs 1061 .. 1100   "1"  (code 0)   no peak                  its baits are dropped from the control set

The chromosome names are chosen so that their codes (the order of np.unique) are NOT the order of their IDs.  Two peaks expand to
nothing: 399 -> 400 (rows 401 .. 405 lie on the next chromosome: the cis clip) and 1099 -> 1100 (rows 1101 .. 1105 lie beyond the
map) — regions that must not be counted."""
import os

import numpy as np

NFRAG = 1100
CHR_RANGES = [("10", 1, 400), ("2", 401, 1000), ("X", 1001, 1060), ("1", 1061, 1100)]
RUEXPAND = 5
EXPECTED_CONTACT = {"10": 120, "2": 590, "X": 2, "1": 0}
#          non-empty regions, cycled in this order ...                                                          ... and the two empty ones
PEAKS = [(140, 255), (406, 991), (1058, 1059), (7, 3), (994, 1000), (203, 180), (700, 650), (301, 330), (1058, 1059)]
EMPTY_PEAKS = [(399, 400), (1099, 1100)]
SHAPES = [1, 63, 64, 65, 255, 257, 4097, 20011]
SEEDS = [1, 2 ** 40 + 12345]


def design():
    """rmap columns (chr, start, end, ID), the baitmap's rows of them, and the per-code tables: names (sorted), chr_of[0 .. NFRAG]
    (-1 = not on the map), chr_min, chr_max, bmap_chr (the baitmap's chromosome as a code of the map)."""
    ids = np.arange(1, NFRAG + 1, dtype=np.int64)
    chrom = np.empty(NFRAG, dtype=object)
    for name, lo, hi in CHR_RANGES:
        chrom[lo - 1:hi] = name
    start = 1 + 4000 * (ids - 1)
    end = start + 3999
    names, codes = np.unique(chrom.astype(str), return_inverse=True)
    chr_of = np.full(NFRAG + 1, -1, dtype=np.int32)
    chr_of[ids] = codes
    chr_min = np.array([ids[codes == c].min() for c in range(len(names))], dtype=np.int32)
    chr_max = np.array([ids[codes == c].max() for c in range(len(names))], dtype=np.int32)
    bait_rows = np.flatnonzero(ids % 7 == 0)
    return dict(ids=ids, chrom=chrom.astype(str), start=start, end=end, names=names, chr_of=chr_of, chr_min=chr_min, chr_max=chr_max,
                bait_rows=bait_rows, bmap_id=ids[bait_rows].astype(np.int32), bmap_chr=codes[bait_rows].astype(np.int32))


def peaks(n_regions):
    """(baitID, oeID) int32 arrays whose expansion holds exactly ``n_regions`` non-empty regions: PEAKS cycled, an empty peak after
    every 50 of them and both at the end."""
    rows = []
    for i in range(n_regions):
        rows.append(PEAKS[i % len(PEAKS)])
        if i % 50 == 49:
            rows.append(EMPTY_PEAKS[(i // 50) % 2])
    rows += EMPTY_PEAKS
    a = np.array(rows, dtype=np.int32)
    return a[:, 0].copy(), a[:, 1].copy()


def ru_rows(n_regions, d=None):
    """The universe of peaks(n_regions) by the literal restatement of getRegionUniverse (post_inputs.region_universe_literal), in
    (regionID, otherEndID) order: int32 columns baitID, regionID, otherEndID.  regionID = 1 + the peak's position, as in the
    reference, so the empty regions' IDs are missing."""
    from post_inputs import region_universe_literal
    d = design() if d is None else d
    pb, po = peaks(n_regions)
    uniq, inverse = np.unique(np.stack([pb, po], 1), axis=0, return_inverse=True)
    rows = region_universe_literal(uniq[:, 0], uniq[:, 1], RUEXPAND, d["chr_of"])
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1]))]
    per = [rows[rows[:, 1] == u + 1] for u in range(len(uniq))]
    out = []
    for i, u in enumerate(np.ravel(inverse)):
        r = per[u].copy()
        r[:, 1] = i + 1
        out.append(r)
    out = np.concatenate(out)
    return tuple(np.ascontiguousarray(out[:, j]) for j in range(3))


def write_files(tmp, d=None):
    """The two design files as chicdiffPipeline() reads them; returns (rmapfile, baitmapfile)."""
    d = design() if d is None else d
    rmapfile, baitmapfile = os.path.join(str(tmp), "ctrl.rmap"), os.path.join(str(tmp), "ctrl.baitmap")
    with open(rmapfile, "w") as f:
        for c, s, e, i in zip(d["chrom"], d["start"], d["end"], d["ids"]):
            f.write(f'"{c}" {s} {e} {i}\n')
    with open(baitmapfile, "w") as f:
        for r in d["bait_rows"]:
            f.write(f'"{d["chrom"][r]}" {d["start"][r]} {d["end"][r]} {d["ids"][r]} "gene{d["ids"][r]}"\n')
    return rmapfile, baitmapfile


def settings(tmp, d=None):
    """The reference's own settings list with only the entries this stage reads replaced."""
    from pipeline_inputs import golden_settings
    rmapfile, baitmapfile = write_files(tmp, d)
    s = golden_settings()
    s["rmapfile"], s["baitmapfile"] = [rmapfile], [baitmapfile]
    s["outprefix"] = [os.path.join(str(tmp), "ctrl")]
    s["RUexpand"] = [RUEXPAND]
    return s
