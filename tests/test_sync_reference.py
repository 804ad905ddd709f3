"""tests/sync_reference.py, the CPU restatement of the flag, page-tag and checksum kernels (csrc/sync.hip), without a GPU: the
numpy-vectorised forms against the plain-integer forms on random inputs, and the integer forms against literals worked out by hand:

page tag (x = seed + page * G; x ^= x >> 29; x *= C; x ^= x >> 32 with C = 0xBF58476D1CE4E5B9)
    page_tag(0, 0): x stays 0 through every step                                                       = 0
    page_tag(1, 0): x = 1; 1 >> 29 = 0; x = C; C >> 32 = 0xBF58476D, low half 0x1CE4E5B9 ^ 0xBF58476D = 0xA3BCA2D4
                                                                                                       = 0xBF58476DA3BCA2D4
    page_tag(2^29, 0): x = 0x20000000 ^ 1 = 0x20000001; x * C = (C << 29) + C mod 2^64 = 0xA39C9CB720000000 + 0xBF58476D1CE4E5B9
                    = 0x62F4E4243CE4E5B9 (the carry out of bit 63 drops); low half 0x3CE4E5B9 ^ 0x62F4E424 = 0x5E10019D
                                                                                                       = 0x62F4E4245E10019D
    the page enters only through seed + page * G mod 2^64: page_tag(s, p) = page_tag((s + p * G) mod 2^64, 0)

checksum (little-endian words, s1 = sum w_i, s2 = sum w_i * (i + 1), a 1 - 3 byte tail one more zero-extended word)
    01 00 00 00 02 00 00 00: words 1, 2                 s1 = 3, s2 = 1 * 1 + 2 * 2 = 5
    01 00 00 00 ff ff:       words 1, 0xFFFF            s1 = 0x10000, s2 = 1 + 2 * 0xFFFF = 0x1FFFF
    ff:                      word 0xFF                  s1 = s2 = 0xFF
    2^17 words of 0xFFFFFFFF: s1 = (2^32 - 1) * 2^17 = 2^49 - 2^17;  sum (i + 1) = 2^16 * (2^17 + 1) = 2^33 + 2^16, so the
                             weighted sum is (2^32 - 1) * (2^33 + 2^16) = 2^65 + 2^48 - 2^33 - 2^16 > 2^64: s2 = 2^48 - 2^33 - 2^16

flags and status
    flag_value(3, 15) = 63; flag_value(4, 0) = 64: the last step of one call is one below the first of the next
    status_code(5, 63) = (5 << 8) | 64 = 1344, decoded back to call 5, flag 63"""
import numpy as np
import pytest

from tests import sync_reference as R

G = 0x9E3779B97F4A7C15


def test_page_tag_literals():
    assert R.page_tag(0, 0) == 0
    assert R.page_tag(1, 0) == 0xBF58476DA3BCA2D4
    assert R.page_tag(1 << 29, 0) == 0x62F4E4245E10019D
    for seed, page in ((0, 1), (2**64 - 1, 1), (0x0123456789ABCDEF, 262146), (2**63, 2**40 + 5)):
        assert R.page_tag(seed, page) == R.page_tag((seed + page * G) % 2**64, 0)
        assert 0 <= R.page_tag(seed, page) < 2**64
    assert R.page_tag(7, 1) != R.page_tag(7, 2) != R.page_tag(8, 2)


def test_page_tags_vectorised_against_the_integers():
    rng = np.random.default_rng(20)
    for seed in [0, 1, 2**64 - 1] + [int(s) for s in rng.integers(0, 2**64, 5, dtype=np.uint64)]:
        pages = np.concatenate([np.arange(0, 300, dtype=np.uint64), rng.integers(0, 2**63, 200, dtype=np.uint64),
                                np.array([262143, 262144, 262146, 2**64 - 1], dtype=np.uint64)])
        got = R.page_tags(seed, pages)
        assert got.dtype == np.uint64 and [int(v) for v in got] == [R.page_tag(seed, int(p)) for p in pages]
        assert [int(v) for v in R.page_tags(seed, 17)] == [R.page_tag(seed, p) for p in range(17)]


def test_checksum_literals():
    assert R.checksum(b"") == (0, 0)
    assert R.checksum(bytes([1, 0, 0, 0, 2, 0, 0, 0])) == (3, 5)
    assert R.checksum(bytes([1, 0, 0, 0, 0xff, 0xff])) == (0x10000, 0x1FFFF)
    assert R.checksum(b"\xff") == (0xFF, 0xFF)
    assert R.words_of(bytes([1, 2, 3, 4, 5, 6, 7])) == [0x04030201, 0x00070605]


def test_checksum_weighted_sum_passes_two_to_the_64():
    data = b"\xff" * (4 * 2**17)
    unwrapped = sum((2**32 - 1) * (i + 1) for i in range(2**17))
    assert unwrapped > 2**64
    assert R.checksum(data) == (2**49 - 2**17, 2**48 - 2**33 - 2**16) == (2**49 - 2**17, unwrapped % 2**64)
    assert R.checksum_np(data) == R.checksum(data)


def test_checksum_vectorised_against_the_integers():
    rng = np.random.default_rng(21)
    for n in list(range(0, 14)) + [255, 256, 257, 1023, 4096 + 2, 4 * 1025 + 3]:
        data = rng.integers(0, 256, n, dtype=np.uint8)
        assert R.checksum_np(data) == R.checksum(data.tobytes()) == R.checksum_np(data.tobytes()), n


def test_swapping_two_unequal_words_changes_s2_only():
    rng = np.random.default_rng(22)
    w = rng.integers(0, 2**32, 64, dtype=np.uint32)
    w[5], w[40] = 0x11111111, 0x22222222
    swapped = w.copy()
    swapped[5], swapped[40] = w[40], w[5]
    a, b = R.checksum(w.tobytes()), R.checksum(swapped.tobytes())
    assert a[0] == b[0] and a[1] != b[1]
    assert (b[1] - a[1]) % 2**64 == ((0x22222222 - 0x11111111) * (6 - 41)) % 2**64


def test_tail_bytes_count_and_later_bytes_do_not():
    body = bytes(range(1, 11))  # 10 bytes: two words and a 2-byte tail
    assert R.checksum(body) != R.checksum(body[:8])                      # the tail is summed
    assert R.checksum(body) == R.checksum(body + b"\0\0")                # ... as a zero-extended word
    assert R.checksum(body) != R.checksum(body[:9] + b"\x7f")            # its last byte matters


def test_flags_and_status():
    assert R.flag_value(3, 15) == 63 and R.flag_value(4, 0) == 64
    assert R.flag_value(2**40, 1) == 2**44 + 1
    assert R.flag_value(2**60, 0) == 0  # (mod 2^64, like the kernel's product)
    assert R.status_code(5, 63) == 1344 and R.decode_status(1344) == (5, 63)
    for call in (0, 1, 2**40 + 3):
        for lane in (0, 31, 63):
            assert R.decode_status(R.status_code(call, lane)) == (call, lane)
    with pytest.raises(AssertionError):
        R.flag_value(1, 16)


# ---- the harness entries of cudecomp_ext.h: what they refuse, and what launches nothing (no call here reaches a device) ------------
def test_entries_refuse_bad_arguments_before_any_launch(capfd):
    import ctypes as C

    import cudecomp_amd as cd
    assert (cd.MAX_FLAGS, cd.FLAG_SCALE) == (R.MAX_FLAGS, R.FLAG_SCALE) == (64, 16)
    L = cd.lib()
    # the header's prototypes against the argtypes the GPU tests call through: as many parameters, pointers at the same positions
    from tests.test_abi import declared_prototypes
    protos = declared_prototypes("cudecomp_ext.h")
    for name in ("cudecompExtSyncEpochBegin", "cudecompExtSyncSignal", "cudecompExtSyncWait", "cudecompExtTagPages",
                 "cudecompExtCheckPages", "cudecompExtChecksum"):
        assert name in cd.EXT_SYMBOLS
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert ["*" in p or p.startswith("hipStream_t") for p in params] == \
               [t is C.c_void_p or hasattr(t, "contents") for t in argtypes], (name, params)
    cells = (C.c_uint64 * 70)()
    at = lambda i: C.addressof(cells) + 8 * i
    flags = lambda n, hole=None: (C.c_void_p * max(n, 1))(*[None if i == hole else at(i) for i in range(n)])
    bad, ok = cd.RESULT_INVALID_USAGE, cd.RESULT_SUCCESS
    epoch, status = at(68), at(69)
    before = (cd.cudecompExtDataLaunchCount(), cd.cudecompExtLastKernelName())
    for n in (-1, 65, 2**31 - 1):
        assert L.cudecompExtSyncEpochBegin(epoch, flags(64), n, None) == bad
        assert L.cudecompExtSyncSignal(epoch, flags(64), n, 0, None) == bad
        assert L.cudecompExtSyncWait(epoch, flags(64), n, 0, status, 0.5, None) == bad
    for step in (-1, 16, 255):
        assert L.cudecompExtSyncSignal(epoch, flags(2), 2, step, None) == bad
        assert L.cudecompExtSyncWait(epoch, flags(2), 2, step, status, 0.5, None) == bad
    for timeout in (0.0, -1.0, 1.0000001, 30.0, float("inf"), float("nan")):   # never more than a second on a flag
        assert L.cudecompExtSyncWait(epoch, flags(1), 1, 15, status, timeout, None) == bad, timeout
    # null pointers where a launch would follow
    assert L.cudecompExtSyncEpochBegin(None, flags(1), 1, None) == bad
    assert L.cudecompExtSyncEpochBegin(None, None, 0, None) == bad          # (n == 0 still bumps the epoch: it is needed)
    assert L.cudecompExtSyncEpochBegin(epoch, None, 1, None) == bad
    assert L.cudecompExtSyncEpochBegin(epoch, flags(64, hole=63), 64, None) == bad
    assert L.cudecompExtSyncSignal(None, flags(1), 1, 15, None) == bad
    assert L.cudecompExtSyncSignal(epoch, flags(3, hole=1), 3, 15, None) == bad
    assert L.cudecompExtSyncWait(None, flags(1), 1, 15, status, 0.5, None) == bad
    assert L.cudecompExtSyncWait(epoch, flags(1), 1, 15, None, 0.5, None) == bad
    assert L.cudecompExtSyncWait(epoch, None, 1, 15, status, 0.5, None) == bad
    assert L.cudecompExtTagPages(None, 4096, 1, None) == bad
    assert L.cudecompExtCheckPages(None, 4096, 1, status, None) == bad
    assert L.cudecompExtCheckPages(epoch, 4096, 1, None, None) == bad
    assert L.cudecompExtChecksum(None, 1, status, None) == bad
    assert L.cudecompExtChecksum(epoch, 1, None, None) == bad
    assert "CUDECOMP:ERROR:" in capfd.readouterr().err
    # nothing to do: success without a launch, nothing written
    assert L.cudecompExtSyncSignal(None, None, 0, 15, None) == ok
    assert L.cudecompExtSyncWait(None, None, 0, 15, None, 1.0, None) == ok
    assert L.cudecompExtTagPages(None, 4095, 1, None) == ok
    assert L.cudecompExtCheckPages(None, 4095, 1, None, None) == ok
    assert L.cudecompExtChecksum(None, 0, None, None) == ok
    assert list(cells) == [0] * 70
    assert (cd.cudecompExtDataLaunchCount(), cd.cudecompExtLastKernelName()) == before


def test_sender_sums_are_indexed_member_destination_two():
    """peerVerifyExchange gathers every member's 2 P sender sums: [member][destination][2].  The body of the end-to-end test says
    so, and a gathered array built that way is read back by sender_sum_index."""
    from tests import sync_bodies as SB
    assert "[member][destination][2]" in SB.verify_exchange_aid.__doc__ and "2 * (s * P + me)" in SB.verify_exchange_aid.__doc__
    P = 4
    mine = lambda member: [v for d in range(P) for v in (1000 * member + 10 * d, 1000 * member + 10 * d + 1)]  # (s1, s2) per destination
    gathered = [v for member in range(P) for v in mine(member)]
    for s in range(P):
        for me in range(P):
            i = SB.sender_sum_index(s, me, P)
            assert gathered[i:i + 2] == [1000 * s + 10 * me, 1000 * s + 10 * me + 1]
