"""Lists of block moves for the batch tests (tests/test_kernel_batches.py on the CPU, tests/test_gpu_kernel_batches.py on the
GPU): the shape strategy of the single-move property sweep (tests/test_gpu_kernels.py draws from the same one), packing of
independently drawn moves into disjoint regions of one source and one destination buffer, the numpy execution of a list one move
after the other, and -- GPU only -- the run of a list through cudecompExtRunMoves with every byte of every destination buffer
compared.  numpy only at import; torch is imported where the device is used."""
import numpy as np

import cudecomp_amd as cd
from oracle import oracle as orc
from tests import accumulate_bodies as AB

# csrc/kernels_batch.h KernelKind, in order: ExtLaunch.kind indexes this
KINDS = ("rows", "rows_shifted", "rows_dense", "transpose", "transpose_window", "transpose_lines", "transpose_rowlines", "generic",
         "rows_add", "generic_add", "rows_fill", "generic_fill")
PAYLOAD = {2: np.uint16, 4: np.uint32, 8: np.uint64, 16: np.complex128}
GUARD = 256  # poison bytes in front of and behind every device buffer (a multiple of every alignment the classifier looks at)


def padded_strides(ext, perm, pad):
    """Strides (elements) of the block `ext` inside a pencil whose memory position i holds logical dim perm[i], rows padded by
    pad[0] and planes by pad[1] rows like halo-carrying pencils; and the pencil's length."""
    shape = [ext[p] for p in perm]
    s_mem = [1, shape[0] + pad[0], (shape[0] + pad[0]) * (shape[1] + pad[1])]
    out = [0, 0, 0]
    for i, p in enumerate(perm):
        out[p] = s_mem[i]
    return out, s_mem[2] * shape[2]


def shape_strategies(st):
    """hypothesis strategies of one randomly drawn move (`st` = hypothesis.strategies): extents 1..150 x 1..70 x 1..12, any
    source / destination permutation, halo-style row and plane padding, element offsets 0..9 (so every alignment)"""
    return dict(ext=st.tuples(st.integers(1, 150), st.integers(1, 70), st.integers(1, 12)),
                sperm=st.permutations((0, 1, 2)), dperm=st.permutations((0, 1, 2)),
                spad=st.tuples(st.integers(0, 5), st.integers(0, 3)), dpad=st.tuples(st.integers(0, 5), st.integers(0, 3)),
                soff=st.integers(0, 9), doff=st.integers(0, 9))


def span(extent, strides):
    return sum((int(e) - 1) * int(s) for e, s in zip(extent, strides)) + 1 if 0 not in tuple(extent) else 0


def cells(extent, strides, off=0):
    """element indices the move touches on one side, dim 0 fastest"""
    if 0 in tuple(extent):
        return np.zeros(0, dtype=np.int64)
    k = np.indices([int(e) for e in extent][::-1]).reshape(3, -1)[::-1]
    return int(off) + k[0] * int(strides[0]) + k[1] * int(strides[1]) + k[2] * int(strides[2])


class Packer:
    """Lays moves one behind the other: every move gets a region of the source buffer (0) and of the destination buffer (1) of
    its own; `gap` spare elements between regions (never written: compared like the poison)."""

    def __init__(self, gap=3, align=1):
        """align: every region starts at a multiple of `align` elements (256: a move then sits at the alignment it has alone)"""
        self.moves, self.len, self.gap, self.align = [], [0, 0], gap, align

    def add(self, extent, ss, ds, soff=0, doff=0, slen=None, dlen=None, row_pitch=0):
        slen = span(extent, ss) if slen is None else slen
        dlen = span(extent, ds) if dlen is None else dlen
        self.moves.append(cd.make_move(extent, ss, ds, self.len[0] + soff, self.len[1] + doff, 0, 1, row_pitch))
        up = lambda n: -(-n // self.align) * self.align
        self.len[0] = up(self.len[0] + soff + slen + self.gap)
        self.len[1] = up(self.len[1] + doff + dlen + self.gap)
        return self.moves[-1]


def reorder(moves, order):
    return [moves[i] for i in order]


def buffer_lengths(moves, bases=False):
    """elements each buffer 0..2 must hold for the list (bases: the destinations live in per-move buffers, see run_list)"""
    n = [0, 0, 0]
    for m in moves:
        if 0 in tuple(m.extent):
            continue
        n[m.src_buf] = max(n[m.src_buf], m.src_off + span(m.extent, m.ss))
        if not bases:
            n[m.dst_buf] = max(n[m.dst_buf], m.dst_off + span(m.extent, m.ds))
    return n


def assert_disjoint_destinations(moves, bases=False):
    """no destination cell belongs to two moves of the list (per destination buffer; with bases every move has its own)"""
    if bases:
        return
    for buf in range(3):
        c = [cells(m.extent, m.ds, m.dst_off) for m in moves if m.dst_buf == buf]
        if c:
            c = np.concatenate(c)
            assert np.unique(c).size == c.size, "destination cells of the list overlap in buffer %d" % buf


def apply_move(mode, dtype, src, dst, m, dst_off, value=None):
    """numpy execution of ONE move on host arrays of the element's payload type (adds: arrays of shape (elements, reals) of the
    reals' bit patterns)"""
    if 0 in tuple(m.extent):
        return
    if mode == cd.MOVES_COPY:
        orc.move3d_reference(src, dst, tuple(m.extent), tuple(m.ss), tuple(m.ds), m.src_off, dst_off)
    elif mode == cd.MOVES_ADD:
        cs, cdst = cells(m.extent, m.ss, m.src_off), cells(m.extent, m.ds, dst_off)
        dst[cdst] = AB.typed_add(dtype, dst[cdst], src[cs])
    else:
        dst[cells(m.extent, m.ds, dst_off)] = value


def host_buffers(moves, es, mode, dtype, seed, bases=False):
    """random bytes for buffers 0..2 (GUARD bytes of poison on both sides) sized for the list; with bases, one more buffer per
    move for its destination.  Returns (list of uint8 arrays for buffers 0..2, list of per-move uint8 arrays or None)."""
    rng = np.random.default_rng(seed)
    make = lambda n: rng.integers(0, 256, 2 * GUARD + n * es, dtype=np.uint8)
    bufs = [make(n) for n in buffer_lengths(moves, bases)]
    own = [make(m.dst_off + span(m.extent, m.ds) + 5) for m in moves] if bases else None
    return bufs, own


def _typed(raw, es, mode, dtype):
    """the elements of a guarded byte buffer as the array apply_move works on (a view)"""
    body = raw[GUARD:raw.size - GUARD]
    if mode == cd.MOVES_ADD:
        return body.view(AB.FORMATS[AB.kind_of(dtype)][0]).reshape(-1, AB.TYPES[dtype][1])
    return body.view(PAYLOAD[es])


def expected_buffers(moves, es, mode, dtype, value, bufs, own):
    """the buffers after the list ran, one move after the other in list order, in numpy"""
    exp = [b.copy() for b in bufs]
    exp_own = [b.copy() for b in own] if own is not None else None
    v = None if value is None or mode != cd.MOVES_FILL else np.frombuffer(value, dtype=PAYLOAD[es])[0]
    for i, m in enumerate(moves):
        src = _typed(exp[m.src_buf], es, mode, dtype)
        dst = _typed(exp_own[i] if own is not None else exp[m.dst_buf], es, mode, dtype)
        apply_move(mode, dtype, src, dst, m, m.dst_off, v)
    return exp, exp_own


def differences(got, want, es, mode, dtype):
    """positions (bytes) where a destination buffer breaks the comparison rule: adds -- an expected NaN real may be ANY NaN
    (tests/test_gpu_halo_accumulate.py), everything else bit for bit; copies and fills and all poison -- byte for byte"""
    if mode != cd.MOVES_ADD:
        return np.flatnonzero(got != want)
    bad = list(np.flatnonzero(got[:GUARD] != want[:GUARD])) + list(got.size - GUARD + np.flatnonzero(got[-GUARD:] != want[-GUARD:]))
    kind = AB.kind_of(dtype)
    u = AB.FORMATS[kind][0]
    g, w = got[GUARD:got.size - GUARD].view(u), want[GUARD:want.size - GUARD].view(u)
    return np.array(bad + list(GUARD + np.flatnonzero(AB.mismatches(kind, g, w)) * np.dtype(u).itemsize), dtype=np.int64)


FAKE = (1 << 32, 1 << 36, 1 << 40)  # 256-byte aligned stand-ins for device addresses (device allocations are aligned so too)


def choice_of(launch):
    """the KernelChoice of a described launch: moves share a launch only when these agree"""
    return tuple(launch[k] for k in ("kind", "es", "vec", "tile_i", "tile_j", "access", "arith"))


def describe_alone(cand, es, mode=cd.MOVES_COPY, dtype=0, flags=0):
    """(choice, workgroups) of the candidate move cand = (extent, ss, ds, soff, doff, row_pitch) launched by itself from
    256-byte aligned buffers, or None when it cannot run (the classifier refuses it)"""
    extent, ss, ds, soff, doff, row_pitch = cand
    try:
        (l,) = describe([cd.make_move(extent, ss, ds, soff, doff, 0, 1, row_pitch)], FAKE, es, mode, dtype, flags)
    except cd.CudecompError:
        return None
    return choice_of(l), l["blocks"]


def groups_by_choice(cands, es, mode=cd.MOVES_COPY, dtype=0, flags=0):
    """{choice: [(workgroups, bytes of the destination span, candidate)]} over the candidates"""
    out = {}
    for c in cands:
        d = describe_alone(c, es, mode, dtype, flags)
        if d is not None:
            out.setdefault(d[0], []).append((d[1], span(c[0], c[2]) * es, c))
    return out


def pick_by_workgroups(group, targets):
    """for every target the member of `group` (groups_by_choice) whose workgroup count is nearest in ratio, the smaller move on a
    tie, no member twice while others are as near"""
    import math
    taken, out = set(), []
    for t in targets:
        best = min(range(len(group)), key=lambda i: (round(abs(math.log(group[i][0] / t)), 2), i in taken, group[i][1]))
        taken.add(best)
        out.append(group[best])
    return out


def row_candidates(es, widths, spad=6, dpad=2, soff=0, doff=0, pitch=False):
    """(w, h, d) blocks cut out of / written into wider pencils; pitch: the moves say that they cover whole rows of the destination"""
    for w in widths:
        for h in (1, 2, 5, 16, 33, 70, 150, 400):
            for d in (1, 2, 3, 7):
                yield ((w, h, d), (1, w + spad, (w + spad) * (h + 1)), (1, w + dpad, (w + dpad) * (h + 2)), soff, doff, w + dpad if pitch else 0)


def describe(moves, addresses, es, mode=cd.MOVES_COPY, dtype=0, flags=0, base_addresses=None):
    return cd.cudecompExtDescribeMoves(moves, addresses, es, mode, dtype, flags, base_addresses)


def run_list(moves, es, mode=cd.MOVES_COPY, dtype=0, value=None, flags=0, bases=False, seed=0, reference_moves=None):
    """GPU: the list through cudecompExtRunMoves from seeded random buffers; EVERY byte of every destination buffer (poison and
    the cells between the moves included) against the numpy execution; launches per class, launches in all and elements per
    class against what cudecompExtDescribeMoves says for the same addresses.  Returns the described launches.
    (reference_moves: another list for the numpy side -- only the test that the comparison can fail passes one.)"""
    import torch
    assert_disjoint_destinations(moves, bases)
    bufs, own = host_buffers(moves, es, mode, dtype, seed, bases)
    exp, exp_own = expected_buffers(moves if reference_moves is None else reference_moves, es, mode, dtype, value, bufs, own)
    dev = [torch.from_numpy(b.copy()).cuda() for b in bufs]
    dev_own = [torch.from_numpy(b.copy()).cuda() for b in own] if bases else None
    assert all(t.data_ptr() % 256 == 0 for t in dev + (dev_own or []))  # (the alignment the lists were composed for)
    ptrs = [t.data_ptr() + GUARD for t in dev]
    base_ptrs = [t.data_ptr() + GUARD for t in dev_own] if bases else None
    want = describe(moves, ptrs, es, mode, dtype, flags, base_ptrs)
    launches, elements, total = cd.cudecompExtRunMoves(moves, ptrs, es, mode, dtype, value, flags, base_ptrs,
                                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    what = (es, mode, dtype, flags, bases, [(l["kind"], l["n"], l["interleave"], l["blocks"]) for l in want])
    assert total == len(want), what
    assert launches == [sum(1 for l in want if l["cls"] == c) for c in range(3)], what
    assert elements == [sum(l["elements"] for l in want if l["cls"] == c) for c in range(3)], what
    assert sum(elements) == sum(int(np.prod(tuple(m.extent))) for m in moves), what
    for name, got, ref in [("buffer %d" % i, dev[i], exp[i]) for i in range(3)] + \
                          ([("destination of move %d" % i, dev_own[i], exp_own[i]) for i in range(len(moves))] if bases else []):
        bad = differences(got.cpu().numpy(), ref, es, mode, dtype)
        assert bad.size == 0, (name, "%d bytes differ, first at byte %d of %d (poison: %d on both sides)"
                               % (bad.size, bad[0], ref.size, GUARD)) + what
    return want
