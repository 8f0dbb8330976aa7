"""Tables as text on the host: the plain-Python twin of the rule above chicdiff_hip_table_text_dev in include/chicdiff_hip.h
(tests/table_text_twin.py) equals DataFrame.to_csv(index=False) byte for byte; the library's double -> text function compiled for the
host equals repr on the float corpus (tests/table_text_inputs.py); chicdiff_amd/csrc/table_text.h compiled on its own equals repr on the
corpus and on two million random bit patterns, also under the address and undefined-behaviour sanitisers; the entry points' refusals
are named.  Everything is compared exactly."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_text_inputs as ti  # noqa: E402
import table_text_twin as tw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    return hip


@pytest.fixture(scope="module")
def corpus_cells():
    """repr of the corpus, once: [bytes] in corpus order (NaN: nothing)."""
    return [tw.float_cell(v) for v in ti.corpus().tolist()]


def test_the_corpus_holds_what_it_says():
    b = ti.corpus_bits()
    v = ti.corpus()
    assert len(b) >= 300_000 and np.isnan(v).sum() >= 8 and np.isinf(v).sum() >= 2
    have = set(b.tolist())
    for x in (0.0, -0.0, 5e-324, 1.7976931348623157e308, 2.2250738585072014e-308, 1e16, 9999999999999998.0, 1e-4, 1e-5, 2.0 ** 53, 2.0 ** -1074,
              2.0 ** 1023, 1e-323, 1e308, 2000.0):
        assert ti.bits(x) in have, x
    assert ti.bits(1e16) - 1 in have and ti.bits(1e-4) - 1 in have and ti.bits(1e-5) - 1 in have
    cells = {tw.float_cell(x) for x in v[:20000].tolist()}
    assert {len(c.lstrip(b"-").replace(b".", b"").split(b"e")[0].strip(b"0")) for c in cells if c and c not in (b"inf", b"-inf")} >= set(range(1, 18))
    assert max(len(c) for c in cells) == 24


@pytest.mark.parametrize("ncol,sep", [(2, ","), (3, "\t"), (5, ","), (8, ","), (8, "\t")])
def test_twin_equals_pandas(ncol, sep):
    n = 3000
    cols = ti.mixed_table(n, ncol, seed=ncol)
    names = [f"c{j}" for j in range(ncol)]
    want = tw.to_frame(cols, names).to_csv(index=False, sep=sep).encode()
    assert tw.header_line(names, sep) + tw.table_text(cols, n, sep) == want


def test_twin_equals_pandas_on_the_whole_float_corpus(corpus_cells):
    import pandas as pd
    v = ti.corpus()
    want = pd.DataFrame({"i": np.arange(len(v), dtype=np.int32), "x": v}).to_csv(index=False).encode().split(b"\n")[1:-1]
    assert [w.split(b",", 1)[1] for w in want] == corpus_cells


def test_twin_equals_pandas_on_a_countput_shaped_table():
    n = 5000
    cols = ti.countput_shaped(n, 3)
    want = tw.to_frame(cols, ti.COUNTPUT_HEADER).to_csv(index=False).encode()
    assert tw.header_line(ti.COUNTPUT_HEADER) + tw.table_text(cols, n) == want


def test_a_one_column_frame_writes_nan_as_two_quotes():
    """Why one-column tables are not offered: the rule's empty cell is not what pandas writes there."""
    import pandas as pd
    got = pd.DataFrame({"x": [1.5, np.nan, 2.0]}).to_csv(index=False)
    assert got == 'x\n1.5\n""\n2.0\n'
    assert pd.DataFrame({"x": [1.5, np.nan, 2.0], "y": [1, 2, 3]}).to_csv(index=False) == "x,y\n1.5,1\n,2\n2.0,3\n"
    with pytest.raises(ValueError, match="2 .. 64 columns"):
        tw.table_text([("float64", np.array([1.5, np.nan]))], 2)


def test_host_selftest_equals_repr_on_the_corpus(lib, corpus_cells):
    assert lib.selftest_format_double(ti.corpus()) == corpus_cells


def test_caps_agree_with_the_header(lib):
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    caps = lib.table_text_caps()
    for name, key in (("ROWS_PER_TILE", "rows_per_tile"), ("LDS_BYTES", "lds_bytes"), ("MAX_COLUMNS", "max_columns"), ("MAX_DICT", "max_dict")):
        assert f"#define CHICDIFF_TABLE_{name} {caps[key]} " in hdr
    assert caps["max_columns"] == tw.MAX_COLUMNS and caps["max_dict"] == tw.MAX_DICT
    assert 2 * caps["lds_bytes"] < 160 * 1024                                  # two workgroups per compute unit
    for sym in ("chicdiff_hip_table_text_dev", "chicdiff_hip_table_write_dev", "chicdiff_hip_table_check", "chicdiff_hip_table_text_caps",
                "chicdiff_hip_selftest_format_double_dev", "chicdiff_hip_selftest_format_double"):
        assert sym in lib.EXPORTS and sym + "(" in hdr


def _build(tmp_path, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", *flags, "-I", os.path.join(ROOT, "chicdiff_amd", "csrc"), os.path.join(ROOT, "tests", "table_text_host.cpp"),
                    "-o", exe], check=True)
    return exe


def _cells(exe, words, mode="double"):
    out = subprocess.run([exe, mode], input=np.ascontiguousarray(words).tobytes(), capture_output=True, check=True).stdout
    return out.split(b"\n")[:-1]


def test_header_on_its_own_equals_repr_and_reads_back(tmp_path, corpus_cells):
    """chicdiff_amd/csrc/table_text.h is host and device code; this is its host half (tests/table_text_host.cpp, built here with the C++
    compiler) on the corpus and on 2 000 000 further random bit patterns: every cell is repr(float) (nothing for NaN), and float(cell)
    has the bits the cell was made from.  The program itself checks tt_double_len against the bytes written and that no byte lands
    outside the cell."""
    exe = _build(tmp_path, "table_text_host", ["-O2"])
    assert _cells(exe, ti.corpus_bits()) == corpus_cells
    rnd = ti.random_bits(2_000_000)
    cells = _cells(exe, rnd)
    vals = rnd.view(np.float64).tolist()
    assert len(cells) == len(vals)
    assert cells == [b"" if v != v else repr(v).encode() for v in vals]
    back = np.array([float(c) if c else 0.0 for c in cells]).view(np.uint64)
    nan = np.isnan(rnd.view(np.float64))
    assert np.array_equal(back[~nan], rnd[~nan]) and nan.sum() > 100
    ints = np.concatenate([np.array([0, -1, 1, 9, 10, -10, 99, 100, 2 ** 31 - 1, -2 ** 31, 2 ** 63 - 1, -2 ** 63], dtype=np.int64),
                           np.random.default_rng(2).integers(-2 ** 63, 2 ** 63 - 1, size=20000, dtype=np.int64),
                           (10 ** np.arange(0, 19, dtype=np.int64)), (10 ** np.arange(0, 19, dtype=np.int64)) - 1])
    assert _cells(exe, ints, "int") == [str(int(v)).encode() for v in ints]


def test_header_on_its_own_under_the_sanitisers(tmp_path, corpus_cells):
    """The same stand-alone program, built with -fsanitize=address,undefined, on the corpus: host code in its own process."""
    exe = _build(tmp_path, "table_text_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert _cells(exe, ti.corpus_bits()) == corpus_cells
    assert _cells(exe, np.array([0, -2 ** 63, 2 ** 63 - 1, -1], dtype=np.int64), "int") == [b"0", b"-9223372036854775808", b"9223372036854775807", b"-1"]


def test_pow10_table_is_what_its_tool_prints():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_pow10_table.py")], capture_output=True, check=True).stdout
    assert out == open(os.path.join(ROOT, "chicdiff_amd", "csrc", "pow10_table.h"), "rb").read()
    assert out.count(b"ull},") == 617


def test_entry_point_refusals_are_named(lib):
    import torch
    i = torch.zeros(3, dtype=torch.int32)
    for entry in (b"a,b", b'a"b', b"a\nb", b"a\rb"):
        with pytest.raises(ValueError, match="dictionary entry 1 holds the separator, a quote or a line break"):
            lib.table_check([i, (None, [b"fine", entry])])
    lib.table_check([i, (None, [b"a,b"])], sep="\t")                            # a comma is no separator here ...
    with pytest.raises(ValueError, match="dictionary entry 0 holds the separator"):
        lib.table_check([i, (None, [b"a\tb"])], sep="\t")                       # ... a tab is
    with pytest.raises(ValueError, match="one-column table is not offered"):
        lib.table_check([torch.zeros(3, dtype=torch.float64)])
    with pytest.raises(ValueError, match="2 .. 64 columns, got 65"):
        lib.table_check([i] * 65)
    lib.table_check([i] * 64)
    with pytest.raises(ValueError, match="1 .. 4096 entries, got 4097"):
        lib.table_check([i, (i, [b"x"] * 4097)])
    with pytest.raises(ValueError, match="1 .. 4096 entries, got 0"):
        lib.table_check([i, (i, [])])
    with pytest.raises(ValueError, match="an entry holds at most 4096 bytes"):
        lib.table_check([i, (i, [b"x" * 4097])])
    with pytest.raises(ValueError, match="a tab, a comma or a blank"):
        lib.table_check([i, i], sep=";")
    lib.table_check([i, (i, [b"x"] * 4096), (None, [b"x" * 4096])])


def test_binding_refusals_are_value_errors(lib):
    import torch
    i = torch.zeros(4, dtype=torch.int32)
    cases = [([i, torch.zeros(4, dtype=torch.float32)], "dtype .* is required, got torch.float32"),
             ([i, torch.zeros(4, dtype=torch.bool)], "dtype .* is required, got torch.bool"),
             ([i, torch.zeros(8, dtype=torch.float64)[::2]], r"columns\[1\]: must be contiguous"),
             ([i, torch.zeros((2, 2), dtype=torch.float64)], "one-dimensional"),
             ([i, torch.zeros(5, dtype=torch.int64)], "4 rows are required, got 5"),
             ([i, np.zeros(4)], "a torch tensor is required"),
             ([i, (torch.zeros(4, dtype=torch.int64), [b"x"])], r"columns\[1\] codes: dtype torch.int32 is required"),
             ([(None, [b"x"]), (None, [b"y"])], "the number of rows is required")]
    for cols, match in cases:
        with pytest.raises(ValueError, match=match):
            lib.table_columns(cols)
    with pytest.raises(ValueError, match="must be on"):
        lib.table_columns([i, i], device=torch.device("cuda", 0))
    arr, n, _ = lib.table_columns([i, (None, ["treated"])])
    assert n == 4 and arr[1].kind == lib.COL_DICT and arr[1].ndict == 1 and not arr[1].d_data


def test_device_write_needs_device_countput():
    from chicdiff_amd import pipeline
    with pytest.raises(ValueError, match="needs device_countput=True"):
        pipeline.getFullRegionData({}, None, None, device_write=True)
