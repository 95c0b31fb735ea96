"""CPU: EmailReveal's inputs from a needle.  The substring search of csrc/zkwg_locate_core.h on the simulated wavefront
against bytes.find and a counting loop, and the host mirror's cut_at_needle against the project's restatement of generatePartialSHA
(the same email with shaPrecomputeSelector = the needle)."""
import random

import pytest

import emailreveal as er
import locatetest as lt

BODY_SHAPE = (576, 192, 0, 1, 12, 1, 0)        # reveal from the body, with the uniqueness check


def _count(src, nd):
    return sum(src[p:p + len(nd)] == nd for p in range(len(src) - len(nd) + 1)) if nd and len(nd) <= len(src) else 0


def _find(src, nd):
    at = src.find(nd) if nd else -1
    return None if at < 0 else at


def _check(src, nd, offset=0, length=None):
    s = src if length is None else src[:length]
    for wave in (False, True):
        assert lt.locate(src, nd, lt.FIRST, wave, offset, length) == _find(s, nd), (wave, len(src), len(nd), offset)
        assert lt.locate(src, nd, lt.COUNT, wave, offset, length) == _count(s, nd), (wave, len(src), len(nd), offset)


def _filler(n, seed=1):
    rng = random.Random(seed)
    return bytes(rng.choice(b"qrstuvw") for _ in range(n))


def test_the_tile_is_what_the_cases_below_assume():
    assert lt.tile() == 1024 and lt.chunk() == 256


@pytest.mark.parametrize("at,total", [(0, 50), (0, 5), (45, 50), (15, 40), (1020, 2000), (1023, 1028), (1024, 1100), (2047, 2100), (2995, 3000)])
def test_needle_at_the_edges_of_lanes_tiles_and_the_source(at, total):
    """at 0, ending at len, across a lane boundary (15 -> 16), across a tile boundary (1,020 -> 1,030), the last position of a tile"""
    nd = b"ABCDE"
    src = bytearray(_filler(total))
    src[at:at + 5] = nd
    assert len(src) == total
    _check(bytes(src), nd)
    _check(bytes(src), nd, offset=3)


@pytest.mark.parametrize("L", [1, 2, 16, 17, 255, 256, 257, 512, 513, 1100])
def test_needle_lengths_up_to_longer_than_a_tile(L):
    rng = random.Random(L)
    nd = bytes(rng.choice(b"ABC") for _ in range(L))
    for at, total in ((0, L), (7, L + 7), (1000, 2500), (1500, L + 1500)):
        src = bytearray(_filler(total))
        src[at:at + L] = nd
        _check(bytes(src), nd)
        _check(bytes(src), nd, offset=5)
    # all of it but the last byte, twice, and then the needle: the chunks after the first decide
    if L > 1:
        near = nd[:-1] + bytes([nd[-1] ^ 1])
        src = near + _filler(9) + near + nd + _filler(30)
        _check(src, nd)
        assert lt.locate(src, nd) == 2 * L + 9


def test_a_source_full_of_the_needles_first_bytes():
    nd = b"abcd"
    src = b"abc" * 64 + nd + b"abc" * 400 + nd + b"ab"
    _check(src, nd)
    assert lt.locate(src, nd) == 192 and lt.locate(src, nd, lt.COUNT) == 2
    assert lt.locate(b"aaab", b"aab") == 1                       # what findIndexInUint8Array misses


def test_overlapping_occurrences_count():
    assert lt.locate(b"aaaaa", b"aaa", lt.COUNT) == 3
    assert lt.locate(b"a" * 2500, b"a" * 300, lt.COUNT) == 2201
    assert lt.locate(b"a" * 2500, b"a" * 300) == 0
    _check(b"ab" * 1200, b"abab")


def test_absent_empty_and_too_long():
    src = _filler(2100)
    _check(src, b"ABC")
    _check(src, b"")
    _check(b"", b"a")
    _check(b"", b"")
    _check(b"abc", b"abcd")
    _check(src, src + b"x")
    _check(src, src)


def test_an_occurrence_that_ends_beyond_the_length_is_none():
    src = _filler(1030) + b"HELLO"
    for length in (1031, 1034):
        _check(src, b"HELLO", length=length)
        assert lt.locate(src, b"HELLO", length=length) is None and lt.locate(src, b"HELLO", lt.COUNT, length=length) == 0
    assert lt.locate(src, b"HELLO", length=1035) == 1030
    src = b"xxHELLO" + _filler(3000, 2) + b"HELLO"
    assert lt.locate(src, b"HELLO", lt.COUNT, length=len(src) - 1) == 1 and lt.locate(src, b"HELLO", lt.COUNT) == 2


@pytest.mark.parametrize("offset", [0, 1, 4, 15])
def test_every_alignment_of_the_base(offset):
    src = bytearray(_filler(2300, 3))
    src[1290:1300] = b"0123456789"
    _check(bytes(src), b"0123456789", offset=offset)
    assert lt.locate(bytes(src), b"0123456789", offset=offset) == 1290


def test_seeded_sweep_over_a_small_alphabet():
    rng = random.Random(2025)
    for _ in range(200):
        src = bytes(rng.choice(b"abc") for _ in range(rng.randrange(0, 3001)))
        L = rng.randrange(1, 49)
        if src and rng.random() < 0.7:           # a piece of the source: present; else most likely absent once L is large
            at = rng.randrange(0, len(src))
            nd = src[at:at + L]
        else:
            nd = bytes(rng.choice(b"abc") for _ in range(L))
        off = rng.randrange(0, 16)
        assert lt.locate(src, nd, lt.FIRST, True, off) == _find(src, nd)
        assert lt.locate(src, nd, lt.COUNT, True, off) == _count(src, nd)


# ------------------------------------------------------------------ the host mirror
def _body(length, marker, at, seed=5):
    from zkwg import synth
    b = bytearray(synth.synthetic_body(random.Random(seed), length).replace(b"~", b"x"))   # ("~~MARK" is lost on the reference's search)
    b[at:at + len(marker)] = marker
    return bytes(b)


@pytest.mark.parametrize("length,at", [(70, 20), (120, 60), (150, 64), (400, 330), (1500, 1410), (2900, 2820), (2900, 2891)])
def test_the_needles_cut_equals_the_selectors_where_the_reference_finds_the_first_occurrence(length, at):
    """(the lengths and positions at which the reference's bodyRemaining, which takes the zero fill up to bodySHALength with it, is
    no longer than maxBodyLength: see the next test)"""
    from zkwg import inputs, synth
    nd = b"~MARK~ER~"
    d = synth.synthetic_dkim_result(3, 0, body=_body(length, nd, at))
    assert d["body"].find(nd) == at == inputs.find_index_in_uint8array(d["body"], nd)
    p = er.reveal_params(BODY_SHAPE)
    got = inputs.generate_email_reveal_inputs_from_dkim_result(d, dict(p, maxSubstringLength=12), needle=nd, cut_at_needle=True)
    ref = inputs.generate_email_reveal_inputs_from_dkim_result(d, dict(p, shaPrecomputeSelector=nd.decode()), needle=nd)
    assert got.keys() == ref.keys()
    for k in ref:
        assert got[k] == ref[k], k
    assert int(got["substringStartIndex"]) == at % 64 and int(got["substringLength"]) == len(nd)
    assert len(got["emailBody"]) == 192


def test_a_cut_that_leaves_exactly_max_body_gives_max_body_bytes():
    """bpad - cut = maxBodyLength: the reference's bodyRemaining is 64 bytes of zero fill longer than the circuit's array there; the
    needle's is the padded body from the cut on and nothing else"""
    from zkwg import inputs, synth
    nd = b"~MARK~ER~"
    d = synth.synthetic_dkim_result(3, 0, body=_body(400, nd, 300))              # bpad = 448, cut = 256
    p = er.reveal_params(BODY_SHAPE)
    got = inputs.generate_email_reveal_inputs_from_dkim_result(d, p, needle=nd, cut_at_needle=True)
    ref = inputs.generate_email_reveal_inputs_from_dkim_result(d, dict(p, shaPrecomputeSelector=nd.decode()), needle=nd)
    assert got["emailBodyLength"] == ref["emailBodyLength"] == "192"
    assert len(got["emailBody"]) == 192 and len(ref["emailBody"]) == 256 and ref["emailBody"][:192] == got["emailBody"]
    assert set(ref["emailBody"][192:]) == {"0"}
    assert all(got[k] == ref[k] for k in ref if k != "emailBody")


def test_aab_behind_aa_the_selector_raises_and_the_needle_succeeds():
    from zkwg import inputs, synth
    body = _body(150, b"aaab", 100)
    assert body.count(b"aab") == 1
    d = synth.synthetic_dkim_result(3, 1, body=body)
    p = er.reveal_params(BODY_SHAPE)
    with pytest.raises(ValueError, match="not found"):
        inputs.generate_email_reveal_inputs_from_dkim_result(d, dict(p, shaPrecomputeSelector="aab"), needle=b"aab")
    got = inputs.generate_email_reveal_inputs_from_dkim_result(d, p, needle=b"aab", cut_at_needle=True)
    assert (got["substringStartIndex"], got["substringLength"], got["emailBodyLength"]) == (str(101 - 64), "3", str(192 - 64))
    assert bytes(int(x) for x in got["emailBody"])[37:40] == b"aab"
    assert got["precomputedSHA"] == [str(x) for x in inputs.partial_sha(body[:64])]


def test_the_mirrors_errors_come_in_the_order_of_the_codes():
    from zkwg import inputs, synth
    gen = inputs.generate_email_reveal_inputs_from_dkim_result
    p = dict(er.reveal_params(BODY_SHAPE), maxSubstringLength=12)
    nd = b"~MARK~ER~"
    d = synth.synthetic_dkim_result(3, 2, body=_body(400, nd, 10))              # so early that the remaining body is too long
    with pytest.raises(ValueError, match="longer than max"):                    # 2
        gen(d, p, needle=nd, cut_at_needle=True)
    with pytest.raises(ValueError, match="does not occur"):                     # 5 before 2
        gen(d, p, needle=b"~ABSENT~", cut_at_needle=True)
    with pytest.raises(ValueError, match="empty or longer"):                    # 7 before 5
        gen(d, p, needle=b"~ABSENT~~~~~~", cut_at_needle=True)
    with pytest.raises(ValueError, match="empty or longer"):
        gen(d, p, needle=b"", cut_at_needle=True)
    with pytest.raises(ValueError, match="Padding to max length"):              # 1 before 7
        gen(d, dict(p, maxHeadersLength=64), needle=b"", cut_at_needle=True)
    with pytest.raises(ValueError, match="refused"):
        gen(d, dict(p, shaPrecomputeSelector="x"), needle=nd, cut_at_needle=True)
    with pytest.raises(ValueError, match="takes a needle"):
        gen(d, p, start=1, length=2, cut_at_needle=True)
    twice = _body(150, nd, 70)
    twice = twice[:100] + nd + twice[109:]
    d2 = synth.synthetic_dkim_result(3, 3, body=twice)
    with pytest.raises(ValueError, match="more than once"):                     # 6
        gen(d2, p, needle=nd, cut_at_needle=True)
    assert gen(d2, dict(p, shouldCheckUniqueness=0), needle=nd, cut_at_needle=True)["substringStartIndex"] == "6"
    # a needle across a soft line break is not in the canonical body: the circuit reveals canonical bytes
    soft = _body(150, b"hel=\r\nlo", 80)
    with pytest.raises(ValueError, match="does not occur"):
        gen(synth.synthetic_dkim_result(3, 4, body=soft), p, needle=b"hello", cut_at_needle=True)
    # the header: found in the header's own bytes, the body prepared as without a needle
    pa = er.reveal_params(er.SHAPES["A"])
    d3 = synth.synthetic_dkim_result(3, 5, body_len=90)
    got = gen(d3, pa, needle=b"message-id:<", cut_at_needle=True)
    assert got == gen(d3, pa, needle=b"message-id:<")
    with pytest.raises(ValueError, match="does not occur"):                     # only in the SHA padding
        gen(d3, pa, needle=b"\x80", cut_at_needle=True)
