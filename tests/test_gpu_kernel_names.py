"""What cudecompExtLastKernelName() says, family by family: one table of small moves (at most 1 MiB each) launched through
cudecompExtMove3D / cudecompExtAccumulate3D with their force flags; after every launch the whole destination is compared with
the numpy restatement of the move (as run_move of tests/test_gpu_kernels.py does) and the name with a literal.  bench.py, the
probes and many tests read that name as "what ran": the literals pin its spelling, template arguments included, for every
kernel a single process can reach -- all four lane widths of the row copy, the shifted and dense row copies, the plain
transposition in every element size and with the longer tiles, the window, lines and row-lines transpositions with cached and
streaming access, the element-wise kernel, the two additions with a real and a complex type.

This table is a sample.  Every instantiation of the LDS-tiled kernels, and the names with the remote-store policy (STREAM 3:
reached on local memory through cudecompExtRunMoves with destination bases), are launched by name in
tests/test_gpu_tiled_kernel_instantiations.py; the multi-rank suites cover the remote launches by their results as well."""
import numpy as np
import pytest
import torch

import cudecomp_amd as cd
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

GENERIC, STREAMING, ALWAYS, WHOLE = 1, 2, 4, 256  # flags of cudecompExtMove3D
PAYLOAD = {2: np.uint16, 4: np.uint32, 8: np.uint64, 16: np.complex128}
REALS = {cd.FLOAT: (np.float32, 1), cd.DOUBLE_COMPLEX: (np.float64, 2)}


def _rows(w, h, d, sp, dp):
    return (w, h, d), (1, sp, sp * (h + 2)), (1, dp, dp * (h + 1))


def _lines(ei, ej, ek, gap):
    """destination rows along j of pitch ej + gap, consecutive k adjacent, slabs i far apart (tests/test_gpu_dense_rows.py)"""
    dk = ej + gap
    return (ei, ej, ek), (1, ei, ei * ej), (dk * (ek + 2), 1, dk)


def _rowlines(ei, ej, ek, gap):
    """destination rows along j of pitch ej + gap, consecutive i adjacent, planes k far apart"""
    di = ej + gap
    return (ei, ej, ek), (1, ei * ek, ei), (di, 1, di * (ei + 2))


DENSE = ((64, 64, 4), (1, 64, 4096), (64, 1, 4096))                # line-aligned everywhere
FAR_SOURCE = ((64, 64, 16), (1, 1024, 64), (64, 1, 4096))          # source rows 16 destination rows apart
ODD = ((71, 67, 5), (1, 71, 71 * 67), (67, 1, 71 * 67))
PADDED_SOURCE = ((64, 64, 2), (1, 66, 66 * 64), (64, 1, 4096))     # source rows off the 128-byte grid, destination on it

# (name, element size or data type, (extent, ss, ds), destination offset in elements, flags)
COPIES = [
    ("rows_kernel<16,0>", 8, _rows(64, 7, 3, 80, 64), 0, 0),
    ("rows_kernel<16,1>", 8, _rows(64, 7, 3, 80, 64), 0, STREAMING),
    ("rows_kernel<8,0>", 8, _rows(7, 9, 5, 7, 7), 0, 0),
    ("rows_kernel<8,1>", 8, _rows(7, 9, 5, 7, 7), 0, STREAMING),
    ("rows_kernel<4,0>", 4, _rows(7, 9, 5, 7, 7), 0, 0),
    ("rows_kernel<4,1>", 4, _rows(7, 9, 5, 7, 7), 0, STREAMING),
    ("rows_kernel<2,0>", 2, _rows(7, 9, 5, 7, 7), 0, 0),
    ("rows_kernel<2,1>", 2, _rows(7, 9, 5, 7, 7), 0, STREAMING),
    ("rows_shifted_kernel<16,0>", 8, _rows(128, 9, 3, 128, 140), 1, ALWAYS),
    ("rows_shifted_kernel<8,1>", 8, _rows(129, 9, 3, 129, 140), 1, ALWAYS | STREAMING),
    ("rows_shifted_kernel<4,0>", 4, _rows(129, 9, 3, 129, 140), 1, ALWAYS),
    ("rows_dense_kernel<0>", 8, _rows(128, 9, 3, 128, 130), 1, WHOLE | ALWAYS),
    ("rows_dense_kernel<1>", 8, _rows(128, 9, 3, 128, 130), 1, WHOLE | ALWAYS | STREAMING),
    ("transpose_kernel<2,8,128,128,0,true>", 2, ((128, 128, 2), (1, 128, 16384), (128, 1, 16384)), 0, 0),
    ("transpose_kernel<2,1,64,64,0,true>", 2, ODD, 0, 0),
    ("transpose_kernel<4,4,64,128,0,true>", 4, DENSE, 0, 0),
    ("transpose_kernel<4,4,64,128,2,true>", 4, DENSE, 0, STREAMING),
    ("transpose_kernel<4,1,64,64,0,true>", 4, ODD, 0, 0),
    ("transpose_kernel<8,2,64,64,0,true>", 8, DENSE, 0, 0),
    ("transpose_kernel<8,2,64,64,2,true>", 8, DENSE, 0, STREAMING),
    ("transpose_kernel<8,2,64,64,4,true>", 8, PADDED_SOURCE, 0, STREAMING),
    ("transpose_kernel<8,1,64,64,0,true>", 8, ODD, 0, 0),
    ("transpose_kernel<8,2,64,128,2,true>", 8, FAR_SOURCE, 0, STREAMING),
    ("transpose_kernel<16,1,32,32,0,false>", 16, DENSE, 0, 0),
    ("transpose_kernel<16,1,32,32,2,false>", 16, DENSE, 0, STREAMING),
    ("transpose_kernel<16,1,32,64,2,false>", 16, FAR_SOURCE, 0, STREAMING),
    ("transpose_window_kernel<4,4,64,128,0>", 4, _lines(64, 256, 3, 2), 1, ALWAYS),
    ("transpose_window_kernel<8,2,64,64,0>", 8, _lines(64, 256, 3, 2), 1, ALWAYS),
    ("transpose_window_kernel<8,1,64,64,4>", 8, _lines(65, 256, 3, 2), 1, ALWAYS | STREAMING),
    ("transpose_window_kernel<16,1,32,32,4>", 16, _lines(32, 256, 3, 2), 1, ALWAYS | STREAMING),
    ("transpose_lines_kernel<4,4,64,128,4,128>", 4, _lines(64, 256, 3, 2), 1, WHOLE | ALWAYS | STREAMING),
    ("transpose_lines_kernel<8,2,64,64,0,128>", 8, _lines(64, 128, 8, 2), 1, WHOLE | ALWAYS),
    ("transpose_lines_kernel<16,1,32,32,0,128>", 16, _lines(32, 256, 3, 2), 1, WHOLE | ALWAYS),
    ("transpose_rowlines_kernel<4,4,64,128,0,128>", 4, _rowlines(64, 321, 3, 2), 1, WHOLE | ALWAYS),
    ("transpose_rowlines_kernel<8,2,64,64,0,128>", 8, _rowlines(64, 161, 3, 2), 1, WHOLE | ALWAYS),
    ("transpose_rowlines_kernel<16,1,32,32,4,128>", 16, _rowlines(64, 81, 3, 2), 1, WHOLE | ALWAYS | STREAMING),
    ("generic_kernel<2,false>", 2, _rows(64, 7, 3, 80, 64), 0, GENERIC),
    ("generic_kernel<4,false>", 4, _rows(64, 7, 3, 80, 64), 0, GENERIC),
    ("generic_kernel<8,false>", 8, _rows(1, 50, 20, 64, 1), 0, 0),   # 1-element rows gathered with a stride
    ("generic_kernel<16,false>", 16, _rows(64, 7, 3, 80, 64), 0, GENERIC),
]
ADDITIONS = [
    ("rows_accumulate_kernel<float,16,0>", cd.FLOAT, _rows(64, 7, 3, 80, 64), 0, 0),
    ("rows_accumulate_kernel<float,4,1>", cd.FLOAT, _rows(7, 9, 5, 7, 7), 0, STREAMING),
    ("rows_accumulate_kernel<double,16,1>", cd.DOUBLE_COMPLEX, _rows(6, 10, 11, 12, 9), 2, STREAMING),
    ("generic_accumulate_kernel<float,1>", cd.FLOAT, _rows(64, 7, 3, 80, 64), 0, GENERIC),
    ("generic_accumulate_kernel<double,2>", cd.DOUBLE_COMPLEX, ODD, 0, 0),   # fastest dims swapped: never a transposing kernel
]


def _span(extent, strides):
    return sum((e - 1) * s for e, s in zip(extent, strides)) + 1


def _launch(launch, what, src, dst0, exp, move, doff, flags, es, name):
    extent, ss, ds = move
    assert _span(extent, ss) * es <= 1 << 20 and _span(extent, ds) * es <= 1 << 20
    d_src, d_dst = torch.from_numpy(src.view(np.uint8)).cuda(), torch.from_numpy(dst0.view(np.uint8)).cuda()
    launch(d_src.data_ptr(), d_dst.data_ptr() + doff * es, what, extent, ss, ds, flags, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), exp.view(np.uint8)), (name, cd.cudecompExtLastKernelName())
    assert cd.cudecompExtLastKernelName() == name


@pytest.mark.parametrize("name,es,move,doff,flags", COPIES, ids=[c[0] for c in COPIES])
def test_copy_kernel_names(name, es, move, doff, flags):
    extent, ss, ds = move
    rng = np.random.default_rng(len(name) + es)
    src = rng.integers(0, 256, (_span(extent, ss) + 16) * es, dtype=np.uint8).view(PAYLOAD[es])
    dst0 = rng.integers(0, 256, (doff + _span(extent, ds) + 16) * es, dtype=np.uint8).view(PAYLOAD[es])
    exp = dst0.copy()
    orc.move3d_reference(src, exp, extent, ss, ds, 0, doff)
    _launch(cd.cudecompExtMove3D, es, src, dst0, exp, move, doff, flags, es, name)


@pytest.mark.parametrize("name,dtype,move,doff,flags", ADDITIONS, ids=[a[0] for a in ADDITIONS])
def test_addition_kernel_names(name, dtype, move, doff, flags):
    extent, ss, ds = move
    real, nc = REALS[dtype]
    es = np.dtype(real).itemsize * nc
    rng = np.random.default_rng(len(name))
    # integers 0..7: every sum is exact; elements are rows of nc reals
    src = rng.integers(0, 8, (_span(extent, ss) + 16, nc)).astype(real)
    dst0 = rng.integers(0, 8, (doff + _span(extent, ds) + 16, nc)).astype(real)
    k = np.indices([int(e) for e in extent]).reshape(3, -1)
    cells = doff + k[0] * ds[0] + k[1] * ds[1] + k[2] * ds[2]
    exp = dst0.copy()
    exp[cells] += src[k[0] * ss[0] + k[1] * ss[1] + k[2] * ss[2]]
    _launch(cd.cudecompExtAccumulate3D, dtype, src, dst0, exp, move, doff, flags, es, name)
