"""What the six kernels of csrc/sync.hip compute, restated from the comments there and in csrc/kernels.h in plain Python integers
masked with 2**64 - 1 -- never by calling the library -- plus numpy-vectorised forms of the page tag and the checksum
(tests/test_sync_reference.py holds the two forms to each other and to literals worked out by hand; tests/test_gpu_sync_kernels.py
holds the kernels to them).  numpy only.

    flag        a flag holds  call * FLAG_SCALE + step:  step 0 = the call has begun, 1 .. 14 = stages landed, 15 = all landed;
                epoch_begin sets call = old epoch + 1 and step 0; wait compares  flag >= call * FLAG_SCALE + step.
    status      a wait that gives up on flag `lane` of call `call` leaves  (call << 8) | (lane + 1);  PeerContext::checkStatus reads it
                back as  call = v >> 8, flag = (v & 0xff) - 1.
    page tag    x = seed + page * 0x9E3779B97F4A7C15;  x ^= x >> 29;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 32   (all mod 2^64), in the
                first 64-bit word of 4-KiB page `page`; only the whole pages of a range carry one.
    checksum    the bytes as little-endian 32-bit words w_0 .. w_(k-1), k = bytes // 4, and -- when bytes % 4 != 0 -- one more word
                w_k made of the 1 - 3 tail bytes, zero-extended:  s1 = sum w_i,  s2 = sum w_i * (i + 1)  (mod 2^64)."""
import numpy as np

MASK = 2**64 - 1
FLAG_SCALE = 16  # kFlagScale
MAX_FLAGS = 64   # kMaxFlags
FLAG_DONE = FLAG_SCALE - 1
PAGE = 4096


def flag_value(call, step):
    assert 0 <= step < FLAG_SCALE
    return (call * FLAG_SCALE + step) & MASK


def status_code(call, lane):
    """what wait_k leaves in the status cell when it gives up on flag `lane`"""
    assert 0 <= lane < MAX_FLAGS
    return ((call << 8) | (lane + 1)) & MASK


def decode_status(value):
    """(call, flag) by the rule of PeerContext::checkStatus"""
    return value >> 8, (value & 0xff) - 1


def page_tag(seed, page):
    x = (seed + page * 0x9E3779B97F4A7C15) & MASK
    x ^= x >> 29
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 32
    return x


def page_tags(seed, pages):
    """page_tag for an array (or a count: pages 0 .. count - 1) of page numbers, as uint64 (numpy's unsigned arithmetic wraps)"""
    page = np.arange(pages, dtype=np.uint64) if np.isscalar(pages) else np.asarray(pages, dtype=np.uint64)
    x = np.uint64(seed & MASK) + page * np.uint64(0x9E3779B97F4A7C15)
    x = x ^ (x >> np.uint64(29))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    return x ^ (x >> np.uint64(32))


def words_of(data):
    """the 32-bit words the checksum runs over, the zero-extended tail word included, as a list of Python integers"""
    raw = bytes(data)
    return [int.from_bytes(raw[i:i + 4], "little") for i in range(0, len(raw), 4)]


def checksum_of_words(words):
    s1 = s2 = 0
    for i, w in enumerate(words):
        s1 = (s1 + w) & MASK
        s2 = (s2 + w * (i + 1)) & MASK
    return s1, s2


def checksum(data):
    """(s1, s2) of a bytes-like object"""
    return checksum_of_words(words_of(data))


def checksum_np(data):
    """the same for a uint8 array (or anything bytes-like), vectorised"""
    raw = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).ravel()
    padded = np.zeros(-(-raw.size // 4) * 4, dtype=np.uint8)
    padded[:raw.size] = raw
    w = padded.view("<u4").astype(np.uint64)
    weight = np.arange(1, w.size + 1, dtype=np.uint64)
    return int(w.sum(dtype=np.uint64)), int((w * weight).sum(dtype=np.uint64))
