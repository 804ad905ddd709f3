"""The six kernels of csrc/sync.hip -- epoch_begin_k, signal_k, wait_k, tag_pages_k, check_pages_k, checksum_k -- launched one at a
time through the harness entries of cudecomp_ext.h (cudecompExtSyncEpochBegin / SyncSignal / SyncWait / TagPages / CheckPages /
Checksum) and compared, exactly, with tests/sync_reference.py, which restates them in plain integers from the comments in the code
(tests/test_sync_reference.py checks it on the CPU); and the debugging aid built on checksum_k, CUDECOMP_DEBUG_VERIFY_EXCHANGE, end
to end.  The bodies are in tests/sync_bodies.py (shapes, memory kinds and their reasons are there).

After every launch every word the launch could have touched is compared together with the sentinels, guards or poison around it;
no launch may move cudecompExtDataLaunchCount or cudecompExtLastKernelName (these are not data movement).  Flags, epoch and status
live in uncached device memory and in registered host memory addressed from the device, as in production.  No wait is asked to
last longer than 0.5 s, and the entry itself refuses more than 1 s.

Every test runs on rank workers of tests/mp.py's pool (the two-stream test: in a fresh process) under a time limit of its own: the
worker is killed when it runs out, so the pytest process never holds the GPU and never waits on it.  Only the 1 GiB page-tag case
allocates more than 16 MiB."""
import pytest

from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

KINDS = ("device", "pinned")


def body(func, args=None, timeout=90):
    return run_ranks(1, "tests.sync_bodies", func, args or {}, timeout=timeout, fresh=False)[0]


@pytest.mark.parametrize("kind", KINDS)
def test_begin_and_signal(kind):
    out = body("flags_begin_signal", {"kind": kind})
    assert out["failures"] == [] and out["launches"] == 2 * 5 * 2 * 5


@pytest.mark.parametrize("kind", KINDS)
def test_wait_already_satisfied(kind):
    """the status cell and everything else stay as they were; between two events no such wait comes near the shortest timeout the
    file uses (0.05 s): at most half of it"""
    out = body("flags_wait_satisfied", {"kind": kind})
    print("slowest satisfied wait: %.6f s" % out["slowest_s"])
    assert out["failures"] == []
    assert out["slowest_s"] < 0.025


@pytest.mark.parametrize("kind", KINDS)
def test_wait_times_out_and_says_which_flag(kind):
    out = body("flags_wait_timeout", {"kind": kind})
    assert out["failures"] == []
    assert len(out["codes"]) == 16 and all(c & 0xff in (1, 32, 64, 8, 41) for c in out["codes"])


@pytest.mark.parametrize("kind", KINDS)
def test_wait_clock_constant(kind):
    """launchWait turns seconds into ticks of the 100 MHz wall clock.  An unsatisfied wait lasts at least its timeout (the loop
    leaves only once the tick difference exceeds it), and the difference between the waits of 0.20 s and 0.05 s is 0.15 s +- 20 %:
    the launch cost cancels, one poll costs one s_sleep(16), microseconds.

    Measured on an MI355X (seconds between two events), two runs: flags in device memory 0.050021 and 0.200018, 0.050021 and
    0.200023; in registered host memory 0.050017 and 0.200015, 0.050020 and 0.200022.  Differences 0.149997 ... 0.150002 s."""
    out = body("wait_clock", {"kind": kind})
    short, long_ = out["seconds"]["0.05"], out["seconds"]["0.20"]
    print("unsatisfied waits, %s memory: %.6f s at 0.05, %.6f s at 0.20, difference %.6f s" % (kind, short, long_, long_ - short))
    assert out["failures"] == []
    assert short >= 0.05 and long_ >= 0.20
    assert 0.15 * 0.8 <= long_ - short <= 0.15 * 1.2


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_advances_one_call_per_replay(kind):
    assert body("graph_replay", {"kind": kind})["failures"] == []


def test_page_tags():
    assert body("page_tags")["failures"] == []


def test_page_tags_second_pass_of_the_capped_grid():
    out = body("page_tags_large", timeout=120)
    assert out["failures"] == [] and out["bad"] == 3


def test_checksum():
    assert body("checksum")["failures"] == []


def test_checksum_tail_bytes():
    """Sums of the 105-element chunk of 2-byte elements and of its twin that differs in the last element only.  Before the tail of
    1 - 3 bytes became a word of its own, checksum_k summed 208 of the 210 bytes and gave both chunks the sums of `without_tail`.

    Measured on an MI355X: the kernel before the fix (behind these same entries) gave 111077801849 / 2893152633517 for BOTH chunks and
    this test failed; the kernel as it is gives 111077822928 / 2893153750704 and, for the twin, 111077855695 / 2893155487355."""
    out = body("checksum_tail")
    print("odd-length chunk: sums %r, twin %r, the first 208 bytes alone %r" % (out["sums"][0], out["sums"][1], out["without_tail"]))
    assert out["failures"] == []
    assert out["sums"][0] != out["sums"][1] and out["without_tail"] not in out["sums"]


def test_the_comparisons_can_fail():
    """the numpy side alone is made wrong, once each, and the comparison must say so for the stated reason; the launches stay the
    valid ones (and pass in the tests above)"""
    out = body("flags_begin_signal", {"kind": "device", "short_reference": True, "ns": [2, 64]})
    # the reference for n - 1 flags against a launch of n: one flag word too many, in every one of the 2 x 2 x 2 x 5 comparisons
    assert len(out["failures"]) == 40 and all(": 1 flag words differ" in f for f in out["failures"]), out["failures"][:3]
    out = body("page_tags", {"page_off_by_one": True, "ps": [1, 257]})
    assert len(out["failures"]) == 6 and all("tag pass" in f and "(page 0)" in f for f in out["failures"]), out["failures"]
    out = body("checksum", {"drop_last_word": True, "sizes": [5, 8, 4 * 257]})
    assert len(out["failures"]) == 6 and all("sums differ" in f for f in out["failures"]), out["failures"]


def test_verify_exchange_aid():
    """CUDECOMP_DEBUG_VERIFY_EXCHANGE=1 on four ranks: the transposes are exact against the numpy references and the aid reports
    nothing -- with chunks of an odd number of 2-byte elements, whose last element the checksums now include.  That the aid ran is
    read from the line it prints per exchange under CUDECOMP_VERBOSE: eight exchanges per rank (two cycles of four transposes), two
    chunks each (the rank's own and its partner's on the 2 x 2 grid), all compared with their senders' sums, none reported."""
    import re
    res = run_ranks(4, "tests.sync_bodies", "verify_exchange_aid", {"gdims": (15, 9, 7), "pdims": (2, 2)}, timeout=180, fresh=False,
                    extra_env={"CUDECOMP_DEBUG_VERIFY_EXCHANGE": "1", "CUDECOMP_VERBOSE": "1"})
    assert len(res) == 4
    for r in res:
        assert r["failures"] == [] and r["lines"] == [], r
        assert len(r["ran"]) == 8, r["ran"]
        ops = [re.fullmatch(r"CUDECOMP: exchange verification rank \d (\w+): 2 chunks summed and compared with their senders' sums, 0 reported", l)
               for l in r["ran"]]
        assert all(ops) and [m.group(1) for m in ops] == ["XToY", "YToZ", "ZToY", "YToX"] * 2, r["ran"]


_two_streams = []


@pytest.mark.parametrize("kind", KINDS)
def test_signal_from_another_stream_releases_the_wait(kind):
    """the one test of the file that is about a process's own state -- which streams it has (tests/sync_bodies.py two_streams) -- so
    its body runs in a fresh process, once for both memory kinds; last in the file, because a fresh launch ends the rank pool"""
    if not _two_streams:
        _two_streams.append(run_ranks(1, "tests.sync_bodies", "two_streams", {"kinds": KINDS}, timeout=120, fresh=True)[0])
    out = _two_streams[0][kind]
    print("%s memory: wait released from the other stream after %.6f s, the signal was done at %.6f s" % (kind, out["seconds"], out["signalled_s"]))
    assert out["failures"] == []
    assert out["seconds"] < 0.5
