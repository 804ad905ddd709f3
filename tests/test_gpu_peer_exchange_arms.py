"""Arms of the one-sided exchanges (csrc/peer_exchange.cc) that no other test of the default suite reaches.

An arm is (entry point, copy engine, where the flags live).  Read from test_gpu_native_sweep.py, test_gpu_relay.py,
test_gpu_transpose.py, test_gpu_halo.py and test_gpu_async.py (ranks share the GPU there, so the library picks the `cu` engine
unless a switch pins it; "-" = the entry point does not use the engine, its copies are kernels on the caller's stream):

    entry point                 cu, board           sdma, board              cu, device flags     sdma, device flags
    peerAlltoall                transpose, async    sweep copy_engines       sweep flags_device   HERE
    peerStagedExchange          transpose, async    sweep seven_stages       sweep flags_device   HERE
    peerPutExchange staged      transpose           -                        sweep flags_device   -
    peerPutExchange direct      transpose           -                        sweep flags_device   -
    two-hop relay               relay               -                        HERE                 -
    halo, plain sequence        halo                sweep copy_engines       sweep flags_device   HERE
    halo, overlapped sequence   sweep overlapped    HERE                     HERE                 HERE

The staged exchange is also run with 3 and with 14 stages on both engines and both flag homes: with more stages wanted than the
chunks have slabs, a stage's slab range [n*k/K, n*(k+1)/K) of a chunk is empty, and the fan-out must still raise that stage's flag.

4 ranks sharing the GPU on a 2 x 2 grid, fp64, 13 x 11 x 7 (uneven chunks, differing send counts), halo 1, periodic; every cell
of every pencil against the closed forms of gpu_bodies.cycle_exact / halo_exact, bit for bit."""
import pytest

import cudecomp_amd as cd
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

GDIMS, PDIMS = (13, 11, 7), (2, 2)
ENGINE = {"cu": {"CUDECOMP_PEER_COPY_ENGINE": "cu"}, "sdma": {"CUDECOMP_PEER_COPY_ENGINE": "sdma"}}
FLAGS = {"board": {}, "device": {"CUDECOMP_FLAGS_IN_DEVICE_MEMORY": "1"}}


def _cycle(backend, env, counter, count=4):
    args = {"gdims": GDIMS, "pdims": PDIMS, "kind": 1, "transpose_backend": backend}
    for r in run_ranks(4, "tests.gpu_bodies", "cycle_exact", args, timeout=120, extra_env=env):
        assert r["failures"] == []
        assert r["counters"][counter] == count, r["counters"]   # the entry point meant really ran, on every hop


def _halos(env):
    args = {"gdims": GDIMS, "pdims": PDIMS, "kind": 1, "halo": (1, 1, 1), "periods": (1, 1, 1), "axes": [0, 1, 2],
            "halo_backend": cd.HALO_COMM_MPI, "check_closed_form_against_oracle": True}
    for failures in run_ranks(4, "tests.gpu_bodies", "halo_exact", args, timeout=120, extra_env=env):
        assert failures == []


def test_all_at_once_exchange_copy_engines_device_flags():
    _cycle(cd.TRANSPOSE_COMM_MPI_P2P, dict(ENGINE["sdma"], **FLAGS["device"]), "peer_barrier")


@pytest.mark.parametrize("flags", ["board", "device"])
@pytest.mark.parametrize("engine", ["cu", "sdma"])
@pytest.mark.parametrize("stages", [3, 14])
def test_staged_exchange(stages, engine, flags):
    env = dict(ENGINE[engine], **FLAGS[flags], CUDECOMP_PIPELINE_MIN_STAGE_MIB="0", CUDECOMP_PIPELINE_STAGES=str(stages))
    _cycle(cd.TRANSPOSE_COMM_NVSHMEM_PL, env, "peer_pipelined")


def test_relay_device_flags():
    _cycle(cd.TRANSPOSE_COMM_NVSHMEM, dict(FLAGS["device"], CUDECOMP_TWO_HOP_RELAY="1"), "relayed")


def test_plain_halo_sequence_copy_engines_device_flags():
    _halos(dict(ENGINE["sdma"], **FLAGS["device"], CUDECOMP_DISABLE_HALO_OVERLAP="1"))


@pytest.mark.parametrize("engine,flags", [("sdma", "board"), ("cu", "device"), ("sdma", "device")])
def test_overlapped_halo_sequence(engine, flags):
    _halos(dict(ENGINE[engine], **FLAGS[flags], CUDECOMP_FORCE_HALO_OVERLAP="1"))
