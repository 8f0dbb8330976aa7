"""f2, text part: the rule both parsers of the library follow (include/chicdiff_hip.h, above chicdiff_hip_chinput_parse_dev), as the
plain-Python twin states it (tests/chinput_twin.py), against the HOST parser on a seeded corpus of mutated bodies — rows or error
offset.  tests/test_chinput_dev_gpu.py holds the device parser to the same twin.  CPU only."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chinput_inputs as ci  # noqa: E402
import chinput_twin as tw  # noqa: E402
from test_chinput import parse  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from chicdiff_amd import hip
    return hip.load_library()


def test_caps(lib):
    from chicdiff_amd import hip
    caps = hip.chinput_caps()
    assert set(caps) == {"tile_bytes", "lane_bytes", "window_bytes"} and all(v > 0 for v in caps.values())
    assert caps["tile_bytes"] % caps["lane_bytes"] == 0 and caps["window_bytes"] > caps["tile_bytes"]


def test_twin_on_written_examples():
    """The rule's corners, by hand."""
    cols = (0, 1, 2)
    assert [a.tolist() for a in tw.parse_body(b"1\t2\t3\n-4 +5,6\tx y\r\n\n\r\n7\t8\t9", cols)[1:]] == [[1, -4, 7], [2, 5, 8], [3, 6, 9]]
    assert tw.parse_body(b"", cols)[0] == "rows" and len(tw.parse_body(b"\n\r\n\n\r", cols)[1]) == 0
    assert tw.parse_body(b"1\t2\t2147483647\n1\t2\t-2147483647\n", cols)[3].tolist() == [2147483647, -2147483647]
    for bad in (b"1\t2\t2147483648", b"1\t2\t-2147483648", b"1\t\t3", b"1\t2", b"1\t2\t", b"1\t-\t3", b"1\t2\t3x", b"1\t2\t3\r\r\n",
                b"1\t2\t+-3", b"1\t2\t 3"):
        assert tw.parse_body(b"5\t6\t7\n" + bad + b"\n8\t9\t10\n", cols) == ("bad", 6), bad
    assert tw.parse_body(b"x\t1\t2\t3\tNA junk\n", (1, 2, 3))[1].tolist() == [1]        # behind the last needed column: not looked at
    assert tw.split_file(b'#c\n#d\n"N",baitID otherEndID\r\n1,2 3\n') == (29, (1, 2, 0))
    assert tw.split_file(b"bait\tN\n")[1] is None


def test_host_parser_equals_twin_on_corpus(lib, tmp_path):
    tile = __import__("chicdiff_amd.hip", fromlist=["hip"]).chinput_caps()["tile_bytes"]
    corpus = ci.corpus(tmp_path)
    clean = bad = bad_beyond = 0
    path = tmp_path / "c.chinput"
    for k, (head, body, cols) in enumerate(corpus):
        want = tw.parse_body(body, cols)
        clean += want[0] == "rows"
        bad += want[0] == "bad"
        bad_beyond += want[0] == "bad" and want[1] >= tile
        path.write_bytes(head + body)
        try:
            got = parse(lib, path, threads=1 + k % 5)
        except ValueError as e:
            m = re.search(r"malformed chinput row at byte offset (\d+) ", str(e))
            assert m, (k, str(e))
            assert want == ("bad", int(m.group(1)) - len(head)), k
            continue
        assert want[0] == "rows", (k, want)
        for a, b in zip(got, want[1:]):
            assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b), k
    # the corpus covers both outcomes, and failures behind the first tile of the device parser (asserted on the twin alone)
    n = len(corpus)
    assert clean >= n / 4 and bad >= n / 4 and bad_beyond >= n / 10, (n, clean, bad, bad_beyond)
