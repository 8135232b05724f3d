"""CPU test of tests/_wide.py: the piecewise reference of the wide-stream GPU tests against the oracle's decoder, with every
stream generator run at a scale of 2^-15 (counts still multiples of 32), where the whole output fits the host."""
import numpy as np
import pytest

from tests import _wide

SHIFT = 15


@pytest.mark.parametrize("case", _wide.GIANT_CASES)
def test_piecewise_expectation_is_the_oracle_decode(oracle, case):
    ws = _wide.giant_case(oracle, case, shift=SHIFT)
    st = ws.stream()
    assert st.size == ws.c_words
    # the region where the case puts it, with groups in front of it that are not a multiple of 1024
    lo, hi = ws.region
    assert np.all(st[lo:hi] & 0x80000000) and not (st[lo - 1] & 0x80000000 and st[lo - 1] & 0x3FFFFFFF > 64)
    assert _wide.TILE_WORDS * (lo // _wide.TILE_WORDS) == lo or case == "C6"
    groups_before = sum(int(x) & 0x3FFFFFFF if x & 0x80000000 else 1 for x in st[:lo])
    assert groups_before % 32 == 0 and groups_before % 1024 != 0
    # (words, groups) and every word
    groups = oracle.decoded_groups(st)
    assert ws.expected() == (oracle.decoded_words(groups), groups)
    assert np.array_equal(ws.expected_host(), oracle.decompress(st))


def test_piece_lookup_and_report(oracle):
    ws = _wide.giant_case(oracle, "C3", shift=SHIFT)
    want = ws.expected_host()
    for i in (0, 3, len(ws.starts) // 2, len(ws.starts) - 1):
        s, n = ws.starts[i], ws.lengths[i]
        assert ws.piece_at(s) == i and ws.piece_at(s + n - 1) == i
        if ws.kinds[i] == "fill":
            assert np.all(want[s: s + n] == ws.values[i])
    assert "piece 0 (word piece" in ws.describe(0)


@pytest.mark.parametrize("extra", [0, 1])
def test_sum_limit_stream(oracle, extra):
    st, (words, groups) = _wide.sum_limit_stream(extra, shift=SHIFT)
    assert st.size == _wide.SUM_LIMIT_FILLS + extra
    assert oracle.decoded_groups(st) == groups and oracle.decoded_words(groups) == words
    full, (_, full_groups) = _wide.sum_limit_stream(extra)
    assert full[0] == _wide.SUM_LIMIT_FILL
    assert (full_groups < 1 << 47) == (extra == 0)


@pytest.mark.parametrize("chunk", [_wide.CHUNK_WORDS, 1000])
def test_checker_finds_the_first_wrong_word(oracle, monkeypatch, chunk):
    """check() on a host tensor: the right output passes; a wrong word -- in a fill piece, a word piece, the last word -- is
    reported by its index and its piece, also where a comparison covers less than one fill (chunk 1000 words)."""
    import torch

    monkeypatch.setattr(_wide, "CHUNK_WORDS", chunk)
    ws = _wide.giant_case(oracle, "C4", shift=SHIFT)
    good = ws.expected_host()
    assert max(ws.lengths) > chunk or chunk == _wide.CHUNK_WORDS
    out = torch.from_numpy(good.view(np.int32).copy())
    assert ws.check(out) == ws.words
    region_piece = ws.region_piece
    assert ws.kinds[region_piece] == "fill" and ws.kinds[region_piece - 1] == "fill" and ws.kinds[1] == "words"
    for at in (ws.starts[region_piece] + 5, ws.starts[region_piece + 64 * 40] + 77, 7, ws.words - 1, ws.starts[1] - 1):
        bad = out.clone()
        bad[at] ^= 1 << 9
        with pytest.raises(AssertionError, match=rf"first wrong word {at} .* in piece {ws.piece_at(at)} "):
            ws.check(bad)
    # two wrong words: the first one is named
    bad = out.clone()
    bad[ws.words - 3] ^= 1
    bad[ws.starts[region_piece] + 2] ^= 1
    with pytest.raises(AssertionError, match=rf"first wrong word {ws.starts[region_piece] + 2} "):
        ws.check(bad)
