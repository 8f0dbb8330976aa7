"""Inputs of the .multimerge tests (tests/test_peaks_merge.py, tests/test_peaks_merge_gpu.py): seeded sets of 2 .. 4 peak matrices that
share some of their keys, and a writer for hand-made rows.  A row is the list of its 11 key fields followed by its score tokens."""
import os

import numpy as np

KEYS = ["baitChr", "baitStart", "baitEnd", "baitID", "baitName", "oeChr", "oeStart", "oeEnd", "oeID", "oeName", "dist"]
SCORE = 5.0
TEXT_CHR = ["chr1", "chr10", "chr2", "chrX", "chr19", "chrY"]     # string order differs from the order of the IDs below
INT_CHR = ["1", "10", "2", "19", "7", "3"]


def write_file(path, names, rows, sep="\t", crlf=False, extra=None):
    """``names``: the score columns; ``extra``: the name of one more column in front of them that is no target."""
    eol = "\r\n" if crlf else "\n"
    with open(path, "w", newline="", encoding="utf-8") as f:
        f.write(sep.join(KEYS + ([extra] if extra else []) + list(names)) + eol)
        for r in rows:
            r = [str(v) for v in r]
            f.write(sep.join(r[:11] + (["0.25"] if extra else []) + r[11:]) + eol)


def key_row(b, oe, chrom, trans=False):
    """The 11 key fields of the pair (bait b, other end oe): everything but the IDs follows from them, so two files agree on a key."""
    names = TEXT_CHR if chrom == "text" else INT_CHR
    bc = names[b % len(names)]
    oc = names[(b + 1) % len(names)] if trans else bc
    pos = lambda i: (i % 500000) * 4000
    dist = "NA" if trans else (str((oe - b) * 4000) if (b + oe) % 2 else "%.1f" % ((oe - b) * 4000 + 0.5))
    return [bc, pos(b), pos(b) + 3999, b, f"gene{b};a", oc, pos(oe), pos(oe) + 3999, oe, "." if oe % 3 else f"oe{oe}", dist]


def fmt(v):
    return "NA" if v != v else "%.6g" % v


def design(F, per_file=2):
    """(chicagoData, targetColumns, the score names of every file).  per_file = 2: file f holds A{f} and B{f}, so with F files each
    condition has F replicates and a key found in one file only fails the replicate rule; per_file = 1 (F = 2): one column per
    condition, no replicate rule."""
    if per_file == 1:
        assert F == 2
        return {"A": {"A0": "a"}, "B": {"B1": "b"}}, ["A0", "B1"], [["A0"], ["B1"]]
    names = [[f"A{f}", f"B{f}"] for f in range(F)]
    chicago = {"A": {f"A{f}": "a" for f in range(F)}, "B": {f"B{f}": "b" for f in range(F)}}
    return chicago, [n for pair in zip(*names) for n in pair], names   # the targets in another order than the files hold them


def make_set(tmp, seed, nrows, overlap="half", chrom="text", per_file=2, shuffle=True, tag="s", **kw):
    """F = len(nrows) files of nrows[f] rows.  overlap: 'none' (disjoint keys), 'all' (file f holds the first nrows[f] of one list of
    keys), 'half' (half of each file from that list, half of its own).  ~6 % trans rows (dist NA, other chromosome); ~8 % adjacent
    other ends; unless overlap is 'all', one bait per file that no other file holds; scores gamma-distributed with ~15 % NA, written with 6 digits.  Returns (paths, chicagoData, targetColumns)."""
    rng = np.random.default_rng(seed)
    F = len(nrows)
    chicago, targets, names = design(F, per_file)
    total = max(nrows) + sum(nrows) + 1
    # distinct (bait, other end) pairs: baits come back, other ends on both sides
    baits = rng.integers(10, 10 + max(total // 4, 8), total)
    pairs, seen = [], set()
    for b in baits:
        while True:
            u = rng.random()
            oe = int(b) + (int(rng.choice([-1, 1])) if u < 0.08 else int(rng.integers(2, 4000)) * int(rng.choice([-1, 1])))
            oe = max(oe, 0)
            if (int(b), oe) not in seen and oe != int(b):
                break
        seen.add((int(b), oe))
        pairs.append((int(b), oe, rng.random() < 0.06))
    shared, own, at = pairs[:max(nrows)], [], max(nrows)
    for n in nrows:
        own.append(pairs[at:at + n])
        at += n
    paths = []
    for f, n in enumerate(nrows):
        k = {"none": 0, "all": n, "half": n // 2}[overlap]
        mine = shared[:k] + own[f][:n - k]
        if n - k >= 1:
            mine[-1] = (900000 + f, 900010 + f, False)                            # a bait that this file alone holds
        if shuffle:
            rng.shuffle(mine)
        rows = []
        for b, oe, trans in mine:
            sc = rng.gamma(2.0, 3.0, len(names[f]))
            sc[rng.random(len(sc)) < 0.15] = np.nan
            rows.append(key_row(b, oe, chrom, trans) + [fmt(v) for v in sc])
        path = os.path.join(str(tmp), f"{tag}{seed}_{f}.txt")
        write_file(path, names[f], rows, extra=f"other{f}", **kw)
        paths.append(path)
    return paths, chicago, targets


# one row whose fields the hand-made cases vary
BASE = ["chr1", 100, 200, 5, "g5", "chr1", 900, 950, 9, ".", "800.5"]


def base_row(scores=("6.5", "7.25"), **kw):
    """BASE with the named key columns replaced, then the score tokens."""
    r = list(BASE)
    for k, v in kw.items():
        r[KEYS.index(k)] = v
    return r + list(scores)
