"""The far-strided streaming transposes whose residency (workgroups per CU) is a launch property: csrc/kernels.cc
residencyPadBytes, dynamic LDS that no kernel references -- the fp64 forward hops launch with 48 KiB per workgroup, the fp64
inverse hops with 96 KiB, the complex128 forward hops with 39.5 KiB.  Moves run through the list entry cudecompExtRunMoves with
flag 2 (streaming regardless of the size); EVERY byte of the destination, a poisoned margin on both sides included, is compared
with numpy applying the move.  Before each run cudecompExtDescribeMove must say that the move takes the path under test and
cudecompExtDescribeResidency that its launch asks for the pad, after it cudecompExtLastKernelName names the kernel that ran.

Forward hops (destination rows far apart, run walk): the smallest move that gets the bench hop's run of 512 tiles, and one
whose run is a divisor of its tile count; for 16-byte elements the smallest with a run of 512 tiles.  Inverse hops (source rows
far apart, 64 x 128 tile): interior tiles, tiles whose upper 64 rows are empty, 16 rows deep, and whose lower 64 rows are 16
deep with the upper empty; each case twice into the same destination with different payloads, so that what one run leaves
behind cannot pass for the next one's result."""
import numpy as np
import pytest

import cudecomp_amd as cd

pytestmark = pytest.mark.gpu

STREAMING = 2
MARGIN = 512  # poisoned elements on both sides of the destination (4 or 8 KiB: the move keeps its alignment)
FORWARD = "transpose_kernel<8,2,64,64,2,true>"
INVERSE = "transpose_kernel<8,2,64,128,2,true>"
FORWARD_16 = "transpose_kernel<16,1,32,32,2,false>"
PAYLOAD = {8: np.dtype("<u8"), 16: np.dtype([("re", "<u8"), ("im", "<u8")])}


@pytest.fixture(scope="module", autouse=True)
def no_rank_pool_beside_this_process():
    """these tests use the GPU from the process that runs them: the rank pool of the multi-rank tests ends first"""
    from tests import mp
    mp.pool_stop()


def span(extent, strides):
    return sum((e - 1) * s for e, s in zip(extent, strides)) + 1


def view(flat, extent, strides):
    """the cells of a move on one side as an array indexed [k, j, i]"""
    return np.lib.stride_tricks.as_strided(flat, shape=extent[::-1], strides=[flat.itemsize * s for s in strides[::-1]])


def random_elements(rng, n, es):
    return rng.integers(0, 1 << 63, n * (es // 8), dtype=np.uint64).view(PAYLOAD[es])


def run_and_compare(extent, ss, ds, check, name, pad, payloads=1, es=8):
    """the move from `payloads` different sources into ONE poisoned destination, one after the other; every byte against numpy"""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(sum(extent))
    want = random_elements(rng, 2 * MARGIN + span(extent, ds), es)  # poison: margins and cells between the rows
    dst = torch.from_numpy(want.view(np.uint64).copy()).cuda()
    move = cd.make_move(extent, ss, ds, 0, MARGIN)
    for p in range(payloads):
        host = random_elements(rng, span(extent, ss), es)
        src = torch.from_numpy(host.view(np.uint64)).cuda()
        d = cd.cudecompExtDescribeMove(src.data_ptr(), dst.data_ptr() + es * MARGIN, es, extent, ss, ds, STREAMING)
        assert (d["cls"], d["access"]) == (1, 2), d
        check(d)
        assert cd.cudecompExtDescribeResidency([move], [src.data_ptr(), dst.data_ptr(), None], es, STREAMING) == [pad]
        assert cd.cudecompExtRunMoves([move], [src.data_ptr(), dst.data_ptr(), None], es, flags=STREAMING, stream=stream)[2] == 1
        torch.cuda.synchronize()
        assert cd.cudecompExtLastKernelName() == name
        view(want[MARGIN:], extent, ds)[...] = view(host, extent, ss)
        bad = np.flatnonzero(dst.cpu().numpy() != want.view(np.uint64))
        assert bad.size == 0, "payload %d: %d words differ, first at %d of %d (margin %d elements)" % (p, bad.size, bad[0], want.size * (es // 8), MARGIN)


@pytest.mark.parametrize("ei,ej,ek", [(64, 1024, 64), (192, 1000, 72)])
def test_forward_hop_with_run_walk(ei, ej, ek):
    def check(d):
        assert (d["variant"], d["tile_i"], d["tile_j"]) == (2, 64, 64) and d["run"] > 1 and d["walk"] == 3, d
        if (ei, ej, ek) == (64, 1024, 64):
            assert d["run"] == 512, d

    run_and_compare((ei, ej, ek), (1, ei, ei * ej), (ej * ek, 1, ej), check, FORWARD, 16 << 10)


def test_complex128_forward_hop_with_run_walk():
    ei, ej, ek = 32, 1024, 32  # 16 MiB, the smallest move of 32 x 32 tiles that gets a run of 512

    def check(d):
        assert (d["variant"], d["tile_i"], d["tile_j"], d["run"], d["walk"]) == (1, 32, 32, 512, 3), d

    run_and_compare((ei, ej, ek), (1, ei, ei * ej), (ej * ek, 1, ej), check, FORWARD_16, 23 << 10, es=16)


@pytest.mark.parametrize("ej", [256, 192, 208, 144])
@pytest.mark.parametrize("ei", [64, 80, 192])
def test_inverse_hop_with_tall_tiles(ei, ej):
    ek = 8 * ej // ei + 1  # the smallest that makes the source rows the far-strided side: ei * ek > 8 * ej
    assert ei * ek > 8 * ej >= ei * (ek - 1)

    def check(d):
        assert (d["variant"], d["tile_i"], d["tile_j"]) == (302, 64, 128), d

    run_and_compare((ei, ej, ek), (1, ei * ek, ei), (ej, 1, ei * ej), check, INVERSE, 32 << 10, payloads=2)
