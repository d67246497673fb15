"""The generic sparse-conv kernels of com_amd/csrc/spconv.hip (gather_gemm_kernel, ggw_kernel, gather_gemm_cls_kernel, wgrad_kernel,
wgrad128_kernel, wgrad_os16_kernel and the slab reductions) against the float64 reference tests/sparse_conv_ref.py, at the edges:
row counts around the 64 / 128 / 192-row tiles, every form of the neighbour-table stride, input rows != output rows, the last input
row at the end of the buffer resource, tables with empty rows / offsets / 16-row groups, device-side row counts over poisoned
capacity-sized buffers, weight gradients cut into several row-range splits over NaN-filled workspaces.

The cases and their inputs come from tests/sparse_conv_ref.py; tests/test_sparse_conv_ref_cpu.py shows (without a GPU) that each of
them tells a dropped pair, a dropped last row, unflipped offsets, a last input row read as zeros and a reused slab from a correct
float32 evaluation.  Tolerances: those of tests/test_gpu_parity.py::_conv_case, now against float64 -- sparse_conv_ref.excess; NO
element of a compared tensor is left out.  What the source claims to be bit-identical is compared bit for bit.

Every judged tensor prints error / tolerance; the worst ratio per kernel family is printed when the module ends (-s)."""
import numpy as np
import pytest
import torch

from tests import kernel_digests as KD
from tests import sparse_conv_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
WORST = {}
SENTINEL = {BF16: 0x7B7B, F32: 0x7B7B7B7B}
UNSUPPORTED = -2


def _ops():
    from com_amd import ops
    return ops


def _L():
    from com_amd import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    print("\nworst error / tolerance per kernel family (test_gpu_sparse_conv_edges.py):")
    for name in sorted(WORST):
        print(f"  {name:<34s} {WORST[name][0]:.4f}   at {WORST[name][1]}")
    # this module fills buffers with NaN, sentinels and garbage indices: hand its cached blocks back to the driver, so that no
    # later test's torch.empty starts from them
    torch.cuda.empty_cache()


def _judge(family, where, got, ref, kind):
    got = got.detach().float().cpu().numpy() if torch.is_tensor(got) else got
    r = R.excess(got, ref, kind)
    key = family + (" " + kind if kind != "wgrad" else "")
    if r > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (r, where)
    print(f"{family:<28s} {where}: error / tolerance {r:.4f}")
    assert r <= 1.0, f"{family} at {where}: error / tolerance = {r:.4f}"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), f"{what}: stored bits differ"


def _sentinel(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    _bits(t).fill_(SENTINEL[dtype])
    return t


def _is_sentinel(t):
    return t.numel() == 0 or bool((_bits(t) == SENTINEL[t.dtype]).all())


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def _pack(w, flip):
    """w [K, cc, co] -> the packed weight of the forward (mode 0) or, for a flipped case, the data-gradient pack (mode 1)"""
    mode = 1 if flip else 0
    return _ops().pack_weight(_dev(R.param_of(w, mode)), mode)


def _raw_gg(x, pw, bias, table, kvol, flip, n_rows_out, c_out, y, n_dev=None, addend=None, bn=None, is_dgrad=None):
    """pcd_sparse_conv_gather_gemm with every buffer the caller's (ops.gather_gemm allocates the output); returns the status."""
    L = _L()
    lib = L.lib()
    bnr = None
    if bn is not None:
        dg = int(bool(flip) or bn.mode == 2) if is_dgrad is None else int(is_dgrad)
        tiles = lib.pcd_sparse_conv_gather_gemm_tiles_dir(x.shape[0], x.shape[1], kvol, n_rows_out, c_out, dg)
        assert tiles > 0
        bnr = bn._struct(tiles, c_out, x.device)
    return lib.pcd_sparse_conv_gather_gemm(L.ptr(x), x.shape[0], x.shape[1], L.ptr(pw), L.ptr(bias), L.ptr(table), table.shape[1], kvol,
                                           int(flip), n_rows_out, L.ptr(n_dev), c_out, L.ptr(y), L.dtype_code(y), L.ptr(addend),
                                           _ops()._byref(bnr), L.stream_ptr())


# =====================================================================================================================================
# gather-GEMM
def _gg_params():
    out = []
    for inst in R.GG_INSTS:
        for form in (("wide", "resident") if inst.wide else ("staged", "resident")):
            out.append(pytest.param(inst, form, id=f"{inst.name} {form}"))
    return out


def _resident_lds(inst):
    """dynamic LDS of the resident form (launch_gg: the whole packed weight + the [K + 1][128] table tile)"""
    nsteps = (inst.kvol * inst.cin + 31) // 32
    return nsteps * (inst.cout // 16) * 1024 + (inst.kvol + 1) * 128 * 4


@pytest.mark.parametrize("inst,form", _gg_params())
def test_gather_gemm_edges(inst, form, pcd_option):
    """Every instantiation gg_dispatch returns, in the staged and the resident form of its width (option "gg_resident_kb"), both output
    dtypes, at 1, tile - 1, tile, tile + 1 and 997 rows with the table strides, row counts, table contents and (bias, addend)
    combinations of sparse_conv_ref.gg_cases.  A resident form that needs more than 160 KB of LDS is refused (PCD_ERR_UNSUPPORTED,
    nothing written).  The wide kernel is also held, bit for bit, to the generic kernel (option "ggw" = 0).  The output buffer is a few
    rows longer than n and holds a sentinel: the rows behind n keep it."""
    ops = _ops()
    resident = form == "resident"
    if form != "wide":
        pcd_option("ggw", 0)
        pcd_option("gg_resident_kb", 1024 if resident else 0)
    refused = resident and _resident_lds(inst) > 160 * 1024
    tile = inst.tile if form == "wide" else R.gg_tile(inst, resident)
    for case in R.gg_cases(inst, tile):
        d = R.gg_data(case)
        n = case.n_out
        assert ops.gather_gemm_is_wide(case.n_in, inst.cin, inst.kvol, n, inst.cout, is_dgrad=inst.flip) == (form == "wide")
        ref = R.ref_gather_gemm(d.x, d.w, d.bias, d.nbr, inst.flip, d.addend)
        x, tab, pw = _dev(d.x, BF16), _dev(d.table), _pack(d.w, inst.flip)
        assert x.shape[0] == case.n_in                                   # (the allocation ends with the last input row)
        bias = _dev(d.bias) if d.bias is not None else None
        for dt in (F32, BF16):
            where = f"{inst.name} {form} n={n} {'f32' if dt == F32 else 'bf16'}"
            add = _dev(d.addend, dt) if d.addend is not None else None
            y = _sentinel((n + 3, inst.cout), dt)
            rc = _raw_gg(x, pw, bias, tab, inst.kvol, inst.flip, n, inst.cout, y, addend=add)
            if refused:
                assert rc == UNSUPPORTED and _is_sentinel(y), where
                continue
            assert rc == 0, (where, rc)
            _judge("ggw_kernel" if form == "wide" else "gather_gemm_kernel", where, y[:n], ref, "f32" if dt == F32 else "bf16")
            assert _is_sentinel(y[n:]), where + ": rows behind n written"
            y2 = _sentinel((n + 3, inst.cout), dt)
            assert _raw_gg(x, pw, bias, tab, inst.kvol, inst.flip, n, inst.cout, y2, addend=add) == 0
            _same_bits(y, y2, where + " second run")
            if dt == F32 and case.kind == "edges" and n >= 3:          # row 1 has no neighbour: bias + addend exactly
                want = np.zeros(inst.cout, np.float32)
                if d.bias is not None:
                    want = want + d.bias
                if d.addend is not None:
                    want = want + d.addend[1]
                assert np.array_equal(y[1].cpu().numpy(), want), where
            if form == "wide":
                pcd_option("ggw", 0)
                assert not ops.gather_gemm_is_wide(case.n_in, inst.cin, inst.kvol, n, inst.cout, is_dgrad=inst.flip)
                y3 = _sentinel((n + 3, inst.cout), dt)
                assert _raw_gg(x, pw, bias, tab, inst.kvol, inst.flip, n, inst.cout, y3, addend=add) == 0
                pcd_option("ggw", 1)
                _same_bits(y, y3, where + " ggw against the generic kernel")


def test_gather_gemm_wide_forward_192_row_tiles_45k_rows():
    """ggw<8,2,3,3,2> in the FORWARD exists between 40 961 and 61 440 rows only: kernel_digests.grid_45k (45 000 rows = 234 tiles of 192 and
    one of 72), against the reference on every row."""
    ops = _ops()
    idx, _, _ = KD.grid_45k()
    assert np.array_equal(idx.cpu().numpy(), R.random_cells(*R.GRID_45K)[0])     # the grid the CPU sensitivity check used
    rb = KD._subm(KD.grid_45k)
    case = R.CASE_45K
    inst, n = case.inst, rb.n_out
    assert n == case.n_out and n % 192 == 72 and 40961 <= n <= 61440
    assert ops.gather_gemm_is_wide(n, 128, 27, n, 128, is_dgrad=False)
    d = R.gg_data(case, rb.nbr_out.cpu().numpy())
    ref = R.ref_gather_gemm(d.x, d.w, d.bias, d.nbr, False)
    x, pw, bias = _dev(d.x, BF16), _pack(d.w, False), _dev(d.bias)
    for dt in (F32, BF16):
        y = _sentinel((n + 3, 128), dt)
        assert _raw_gg(x, pw, bias, rb.nbr_out, 27, False, n, 128, y) == 0
        _judge("ggw_kernel", f"{inst.name} {'f32' if dt == F32 else 'bf16'}", y[:n], ref, "f32" if dt == F32 else "bf16")
        assert _is_sentinel(y[n:])


@pytest.mark.parametrize("inst", [pytest.param(i, id=i.name) for i in R.DEVCOUNT_INSTS])
def test_gather_gemm_device_side_count(inst):
    """Static-shape mode: the host passes a capacity (1.25 x n rounded to 4), the row count lives on the device.  n_dev = 0, 1 and tile + 1;
    the output buffer and the addend's tail hold a sentinel, the table columns behind n_dev hold garbage -- negative and out-of-range
    indices included.  A kernel that used one would fetch it with a raw buffer load, whose DOCUMENTED answer to an offset beyond
    num_records is zeros without a memory access (the kernels rely on it for every missing neighbour): this is no provoked fault, and
    the kernels must not use such an entry anyway.  Rows < n_dev match the reference and the launch with the same count given from the
    host bit for bit; rows >= n_dev are untouched; with n_dev = 0 nothing is written."""
    cap = R.capacity(inst.tile + 1)
    fam = "ggw_kernel" if inst.wide else "gather_gemm_kernel"
    for nd, case in R.devcount_cases(inst):
        assert case.stride == cap and nd < cap
        d = R.gg_data(case)
        if nd == 0:
            d.table[:, 0] = R.GARBAGE[1]
        x, tab, pw, bias = _dev(d.x, BF16), _dev(d.table), _pack(d.w, inst.flip), _dev(d.bias)
        ref = R.ref_gather_gemm(d.x, d.w, d.bias, d.nbr, inst.flip, d.addend)[:nd]
        for dt in (F32, BF16):
            where = f"{inst.name} n_dev={nd} of {cap} {'f32' if dt == F32 else 'bf16'}"
            add = _sentinel((cap, inst.cout), dt)
            add[:nd] = _dev(d.addend, dt)[:nd]
            y = _sentinel((cap, inst.cout), dt)
            assert _raw_gg(x, pw, bias, tab, inst.kvol, inst.flip, cap, inst.cout, y, n_dev=_i32(nd), addend=add) == 0, where
            assert _is_sentinel(y[nd:]), where + ": rows >= n_dev written"
            if nd == 0:
                continue
            _judge(fam, where, y[:nd], ref, "f32" if dt == F32 else "bf16")
            yh = _sentinel((cap, inst.cout), dt)
            assert _raw_gg(x, pw, bias, tab, inst.kvol, inst.flip, nd, inst.cout, yh, addend=add) == 0, where
            _same_bits(y, yh, where + " device against host count")


def _bn_expect(out, n, bn):
    """float64 column sums a BnReduce of `bn.mode` takes over the first n rows of the STORED output"""
    o = out[:n].double().cpu()
    if bn.mode == 1:
        return o.sum(0), (o * o).sum(0)
    dz = o * (bn.y[:n].double().cpu() > 0) if bn.relu else o
    xhat = (bn.x[:n].double().cpu() - bn.mean.double().cpu()) * bn.invstd.double().cpu()
    return dz.sum(0), (dz * xhat).sum(0)


@pytest.mark.parametrize("inst,mode", [pytest.param(i, m, id=f"{i.name} mode {m}") for i, m in R.BN_CASES])
def test_gather_gemm_bn_reductions_at_a_partial_tile(inst, mode):
    """PcdBnReduce modes 1 and 2 with a partial last tile (tile + 1 rows), the count from the host and from the device (capacity
    1.25 x): the partial rows summed in float64 equal the float64 column sums of the stored output (tolerance of
    test_conv_epilogue_takes_batchnorm_reductions: 2e-5 of the largest sum + 1e-4), the rows of the surplus tiles are exact zeros and
    the output is the plain launch's, bit for bit."""
    ops = _ops()
    n = inst.tile + 1
    c = inst.cout
    rng = np.random.default_rng(9500 + R.GG_INSTS.index(inst))
    for count_on_device in (False, True):
        case = R.bn_case(inst, mode, count_on_device)
        rows = case.stride
        assert case.n_out == n and rows == (R.capacity(n) if count_on_device else n)
        d = R.gg_data(case)
        x, tab, pw, bias = _dev(d.x, BF16), _dev(d.table), _pack(d.w, inst.flip), _dev(d.bias)
        add = None
        if d.addend is not None:
            add = _sentinel((rows, c), BF16)
            add[:n] = _dev(d.addend, BF16)
        n_dev = _i32(n) if count_on_device else None
        bx = torch.full((rows, c), float("nan"), dtype=BF16, device=DEV)
        by = torch.full((rows, c), float("nan"), dtype=BF16, device=DEV)
        bx[:n], by[:n] = _dev(R.normal_bf16(rng, n, c), BF16), _dev(np.maximum(R.normal_bf16(rng, n, c), 0), BF16)
        mean, invstd = _dev(rng.standard_normal(c).astype(np.float32) * 0.3), _dev(rng.random(c).astype(np.float32) + 0.5)
        bn = ops.BnReduce(1) if mode == 1 else ops.BnReduce(2, True, x=bx, y=by, mean=mean, invstd=invstd)
        assert bn.usable(c, BF16)
        where = f"{inst.name} mode {mode} {'device' if count_on_device else 'host'} count"
        y = _sentinel((rows, c), BF16)
        assert _raw_gg(x, pw, bias, tab, inst.kvol, inst.flip, rows, c, y, n_dev=n_dev, addend=add, bn=bn) == 0, where
        plain = _sentinel((rows, c), BF16)
        assert _raw_gg(x, pw, bias, tab, inst.kvol, inst.flip, rows, c, plain, n_dev=n_dev, addend=add) == 0, where
        _same_bits(y, plain, where)
        assert _is_sentinel(y[n:])
        ref = R.ref_gather_gemm(d.x, d.w, d.bias, d.nbr, inst.flip, d.addend)
        _judge("ggw_kernel" if inst.wide else "gather_gemm_kernel", where, y[:n], ref, "bf16")
        part = bn.partial_keep if bn.partial_keep is not None else bn.partial       # [tiles, 2, c], one row per workgroup
        live = -(-n // inst.tile)
        assert part.shape[0] >= 8 and live == 2
        assert bool((part[live:] == 0).all()), where + ": surplus tile rows"
        for got, want, what in zip((part[:, 0], part[:, 1]), _bn_expect(y, n, bn), ("first sum", "second sum")):
            err = float((got.double().sum(0).cpu() - want).abs().max())
            assert err <= 2e-5 * (float(want.abs().max()) + 1e-6) + 1e-4, (where, what, err)
        if bn.partial_keep is not None:                                            # the 16 "mid" rows folded inside the launch
            for q, want in enumerate(_bn_expect(y, n, bn)):
                err = float((bn.partial[:, q].sum(0).cpu() - want).abs().max())
                assert err <= 2e-5 * (float(want.abs().max()) + 1e-6) + 1e-4, (where, "mid", q, err)


def _small_grid():
    return KD.random_grid(*R.SMALL_GRID)


def test_gather_gemm_packed_table_equals_full_table():
    """The packed output-side table of a strided conv (pcd_sparse_conv_gather_gemm_packed) against the full table: same bits, both
    against the reference; the wide kernel stages full tables only and refuses a packed one."""
    ops = _ops()
    L = _L()
    full, comp = KD._compact_pair(_small_grid, "edges1499")
    m = full.n_out
    assert comp.nbr_out_packed is not None and int(comp.n_out_dev.item()) == m
    nbr = full.nbr_out.cpu().numpy()
    n_in = full.n_in
    assert np.array_equal(nbr, R.oracle_strided(R.random_cells(*R.SMALL_GRID)[0], R.SMALL_GRID[2:5], yxz=True)[1])
    assert np.array_equal(_small_grid()[0].cpu().numpy(), R.random_cells(*R.SMALL_GRID)[0])
    for cin, cout, seed in R.PACKED_WIDTHS:
        d = R.gg_data(R.packed_case(cin, cout, seed, n_in, m), nbr)
        ref = R.ref_gather_gemm(d.x, d.w, d.bias, d.nbr, False, d.addend)
        x, pw, bias = _dev(d.x, BF16), _pack(d.w, False), _dev(d.bias)
        for dt in (F32, BF16):
            add = _dev(d.addend, dt)
            yf = ops.gather_gemm(x, pw, bias, full.nbr_out, 27, False, m, cout, dt, addend=add)
            addp = torch.zeros((comp.n_out, cout), dtype=dt, device=DEV)
            addp[:m] = add
            yp = ops.gather_gemm(x, pw, bias, comp.nbr_out_packed, 27, False, comp.n_out, cout, dt, addend=addp, nbr_packed=True,
                                 n_dev=comp.n_out_dev)
            _same_bits(yf, yp[:m], f"packed {cin}->{cout}")
            _judge("gather_gemm_kernel", f"packed {cin}->{cout} {'f32' if dt == F32 else 'bf16'}", yp[:m], ref,
                   "f32" if dt == F32 else "bf16")
    x = torch.zeros((n_in, 128), dtype=BF16, device=DEV)
    pw = ops.pack_weight(torch.zeros((64, 27, 128), device=DEV), 0)
    y = _sentinel((comp.n_out, 64), BF16)
    rc = L.lib().pcd_sparse_conv_gather_gemm_packed(L.ptr(x), n_in, 128, L.ptr(pw), None, L.ptr(comp.nbr_out_packed),
                                                    comp.nbr_out_packed.shape[1], 27, comp.n_out, L.ptr(comp.n_out_dev), 64, L.ptr(y),
                                                    L.dtype_code(y), None, None, L.stream_ptr())
    assert rc == UNSUPPORTED and _is_sentinel(y)


@pytest.mark.parametrize("gname,idx,batch,shape", [pytest.param(*g, id=g[0]) for g in R.class_grids()])
def test_dgrad_classes_on_edge_grids(gname, idx, batch, shape):
    """gather_gemm_cls_kernel (the data gradient of a strided conv over parity-class row groups) on a single voxel, on a grid whose
    voxels all fall into one class, and on a prime row count: bit-equal to gather_gemm over nbr_in with and without addend, both
    against the reference."""
    ops = _ops()
    rb = ops.rulebook_conv(_dev(idx), batch, shape, 3, 2, 1)
    assert rb.classes is not None and rb.n_in == idx.shape[0]
    n = rb.n_in
    if gname == "one parity class":
        assert len(np.unique(idx[:, 1:] % 2, axis=0)) == 1
    nbr_in = rb.nbr_in.cpu().numpy()
    assert np.array_equal(nbr_in, R.oracle_strided(idx, shape)[0])         # the table the CPU sensitivity check used
    for c_dy, c_in, seed in R.CLASS_WIDTHS:
        d = R.gg_data(R.class_case(c_dy, c_in, seed, n, rb.n_out), nbr_in)
        dy, pd = _dev(d.x, BF16), _pack(d.w, True)                 # (data-gradient pack; the table is input-side: no flip)
        for dt in (F32, BF16):
            for addend in (None, d.addend):
                add = _dev(addend, dt) if addend is not None else None
                where = f"{gname} {c_dy}->{c_in} {'f32' if dt == F32 else 'bf16'}{' +addend' if add is not None else ''}"
                got = ops.dgrad_classes(dy, pd, rb, c_in, dt, addend=add)
                gen = ops.gather_gemm(dy, pd, None, rb.nbr_in, 27, False, n, c_in, dt, addend=add)
                _same_bits(got, gen, where)
                _judge("gather_gemm_cls_kernel", where, got, R.ref_gather_gemm(d.x, d.w, None, d.nbr, False, addend),
                       "f32" if dt == F32 else "bf16")


# =====================================================================================================================================
# weight gradient
def _raw_wgrad(case, d, *, shift_out=False, count_on_device=False, host_rows=None):
    """pcd_sparse_conv_wgrad_v2 + pcd_sparse_conv_wgrad_reduce over a NaN-filled workspace of the test's own and a NaN-filled dW.
    shift_out: dW is a view one float behind a 16-byte boundary (the scalar reduction).  count_on_device: n_x is the capacity, the row
    count (case.n_x_dev) a device scalar and the x rows behind it NaN.  host_rows: n_x = that many rows, from the host.
    Returns (status, dW [cout, K, cin] or None, workspace as floats)."""
    L = _L()
    lib = L.lib()
    K = len(case.counts)
    x = _dev(d.x, BF16)
    n_x, n_x_dev = case.n_x, None
    if count_on_device:
        x[case.n_x_dev:] = float("nan")
        n_x_dev = _i32(case.n_x_dev)
    if host_rows is not None:
        x, n_x = x[:host_rows].contiguous(), host_rows
    dy, pairs, num = _dev(d.dy, BF16), _dev(d.pairs), _dev(d.pair_num)
    wsb = int(lib.pcd_sparse_conv_wgrad_workspace_bytes(K, case.cin, case.cout, case.pmax))
    assert wsb > 0 and wsb % 4 == 0
    ws = torch.full((wsb // 4,), float("nan"), dtype=F32, device=DEV)
    n = case.cout * K * case.cin
    buf = torch.full((n + 8,), float("nan"), dtype=F32, device=DEV)
    dw = buf[1:1 + n] if shift_out else buf[:n]
    assert (dw.data_ptr() % 16 != 0) == shift_out
    rc = lib.pcd_sparse_conv_wgrad_v2(L.ptr(x), n_x, L.ptr(n_x_dev), case.cin_pad, case.cin, L.ptr(dy), case.n_dy, case.cout, L.ptr(pairs),
                                      L.ptr(num), K, case.pmax, L.ptr(dw), L.ptr(ws), wsb, L.stream_ptr())
    if rc != 0:
        return rc, None, ws
    rc = lib.pcd_sparse_conv_wgrad_reduce(K, case.cin, case.cout, case.pmax, L.ptr(dw), L.ptr(ws), L.stream_ptr())
    assert bool(torch.isnan(buf[n + (1 if shift_out else 0):]).all()), "written behind dW"
    return rc, dw.view(case.cout, K, case.cin), ws


def _wg_options(case, pcd_option):
    pcd_option("wg_rows", R.WG_ROWS)
    if "wg128=0" in case.name:
        pcd_option("wg128", 0)
    if case.wg128_chunks:
        pcd_option("wg128_chunks", case.wg128_chunks)


def _wg_check(family, case, pcd_option, **kw):
    _wg_options(case, pcd_option)
    d = R.wg_data(case)
    ref = R.ref_wgrad(d.x, d.dy, d.pairs, d.pair_num, case.cin)
    rc, dw, ws = _raw_wgrad(case, d, **kw)
    assert rc == 0, (case.name, rc)
    assert dw.shape == (case.cout, len(case.counts), case.cin)
    _judge(family, case.name, dw, ref, "wgrad")
    rc, dw2, _ = _raw_wgrad(case, d, **kw)
    assert rc == 0
    _same_bits(dw.contiguous(), dw2.contiguous(), case.name + " second run")
    return d, ref, dw, ws


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.WG_KERNEL_CASES])
def test_wgrad_kernel_instantiations(case, pcd_option):
    """All nine wgrad_kernel<MB, NBW> (cin, cout in {16, 32, 64}), the multi-chunk forms (128 x 64, 64 x 128, 128 x 128 under "wg128" = 0),
    5 real input channels in rows of 8, and the widths the entry point accepts but no layer uses -- cout = 24 and 40 (cout % 16 == 8) and
    cin_pad = 24: the kernel guards every 16-byte piece of a staged row with `c < cout` / `c < cin_pad` and every slab store with
    `co < cout` / `ci < cin`, so they are CORRECT against the reference, not refused.  523 input rows in 3 splits (2 where the layer has
    4 or more channel chunks); the offsets hold 0, 1, 32, 33, ... and all 523 rows."""
    splits, _ = R.split_plan(case.n_x, case.pmax, case.cin, case.cout, R.WG_ROWS)
    assert splits in (2, 3)
    _wg_check("wgrad_kernel", case, pcd_option)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.WG_SPLIT_CASES])
def test_wgrad_kernel_splits(case, pcd_option):
    """Option "wg_rows" = 256: 2 to 11 row-range splits at 257 to 2503 input rows -- the 32-ary lower-bound search (0, 1, 2 and 3 rounds:
    0, 1 / 32, 33 / 1024 and 1025 pairs per offset), the split boundaries, pmax above the row count, the count on the device below the
    capacity (the ranges follow the device count: bit-equal to the same count from the host), and a pair list whose input rows all
    fall into ONE split: every other slab is written as zeros (the NaN poison shows a slab that was skipped)."""
    dev_count = case.n_x_dev is not None
    d, ref, dw, ws = _wg_check("wgrad_kernel", case, pcd_option, count_on_device=dev_count)
    splits, _ = R.split_plan(case.n_x, case.pmax, case.cin, case.cout, R.WG_ROWS)
    slab = ws[:splits * ref.size].view(splits, -1)
    assert ws.numel() == splits * ref.size and bool(torch.isfinite(slab).all()), case.name + ": a slab was not written"
    if dev_count:
        rc, dwh, _ = _raw_wgrad(case, d, host_rows=case.n_x_dev)
        assert rc == 0
        _same_bits(dw.contiguous(), dwh.contiguous(), case.name + " device against host count")
    if case.row_range is not None:
        per = -(-case.n_x // splits)
        own = case.row_range[0] // per
        assert (case.row_range[1] - 1) // per == own
        for q in range(splits):
            if q != own:
                assert bool((slab[q] == 0).all()), f"{case.name}: slab {q} is not zero"
        _judge("wgrad_kernel", case.name + " own slab", slab[own].view(ref.shape), ref, "wgrad")


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.WG128_CASES])
def test_wgrad128_kernel(case, pcd_option):
    """cin = cout = cin_pad = 128: kvol 1, 8 and 27; about 100 pairs against 512 chunks and against 8 ("wg128_chunks"); an offset with no
    pair; a pair list of one pair; 2003 pairs (a prime) -- over a NaN-filled tile workspace."""
    _wg_check("wgrad128_kernel", case, pcd_option)


def test_wgrad_reductions_scalar_and_empty(pcd_option):
    """wgrad_reduce_kernel<1>: dW one float behind a 16-byte boundary; pmax == 0: a zeroed dW and no reduction."""
    case = R.WG_KERNEL_CASES[4]
    _wg_check("wgrad_reduce_kernel<1>", case, pcd_option, shift_out=True)
    L = _L()
    lib = L.lib()
    dw = torch.full((16 * 27 * 16,), float("nan"), dtype=F32, device=DEV)
    x = torch.zeros((4, 16), dtype=BF16, device=DEV)
    assert lib.pcd_sparse_conv_wgrad_v2(L.ptr(x), 4, None, 16, 16, L.ptr(x), 4, 16, None, None, 27, 0, L.ptr(dw), None, 0,
                                        L.stream_ptr()) == 0
    assert lib.pcd_sparse_conv_wgrad_reduce(27, 16, 16, 0, L.ptr(dw), None, L.stream_ptr()) == 0
    assert bool((dw == 0).all())


def test_wgrad_batched_reduction_equals_single_jobs(pcd_option):
    """One wgrad_reduce_batched_kernel launch for the deferred jobs of several layers (a split wgrad_kernel job, the scalar-store
    5-channel one, a wgrad128 job, a pmax = 0 job) equals the single-job results bit for bit."""
    ops = _ops()
    pcd_option("wg_rows", R.WG_ROWS)
    cases = (R.WG_KERNEL_CASES[4], R.WG_KERNEL_CASES[12], R.WG128_CASES[1], R.WG_SPLIT_CASES[2])
    jobs, deferred, single, refs = [], [], [], []
    for case in cases:
        d = R.wg_data(case)
        x, dy, pairs, num = _dev(d.x, BF16), _dev(d.dy, BF16), _dev(d.pairs), _dev(d.pair_num)
        K = len(case.counts)
        single.append(ops.wgrad(x, case.cin, dy, pairs, num, K).clone())
        deferred.append(ops.wgrad(x, case.cin, dy, pairs, num, K, defer=jobs))
        refs.append(R.ref_wgrad(d.x, d.dy, d.pairs, d.pair_num, case.cin))
    x, dy = torch.zeros((4, 32), dtype=BF16, device=DEV), torch.zeros((4, 32), dtype=BF16, device=DEV)
    empty = ops.wgrad(x, 32, dy, torch.empty((27, 2, 0), dtype=torch.int32, device=DEV), torch.zeros(27, dtype=torch.int32, device=DEV),
                      27, out=torch.full((32, 27, 32), float("nan"), device=DEV), defer=jobs)
    assert len(jobs) == len(cases) + 1 and jobs[-1].pmax == 0
    ops.wgrad_reduce_batched(jobs)
    for case, a, b, ref in zip(cases, deferred, single, refs):
        _same_bits(a, b, case.name + " batched against single")
        _judge("wgrad_reduce_batched_kernel", case.name, a, ref, "wgrad")
    assert bool((empty == 0).all())


@pytest.mark.parametrize("case", [pytest.param(c, id=f"cin_pad={c.cin_pad} n={c.n_out} of {c.cap}") for c in R.OS_CASES])
def test_wgrad_output_stationary(case):
    """wgrad_os16_kernel through ops.wgrad(nbr_out=..., n_out_dev=...): kvol 27, cout 16, cin_pad 8 (5 real channels) and 16, at 1, 1023,
    1024 and 1025 output rows (1024 per workgroup), the count on the device below the capacity with NaN in dy's tail and garbage in
    the table's: against the reference, twice the same bits, and the same bits as the count given from the host."""
    ops = _ops()
    x_np, dy_np, table = R.os_data(case)
    n = case.n_out
    ref = R.ref_wgrad_table(x_np, np.nan_to_num(dy_np), table, n, case.cin)
    x, dy, tab = _dev(x_np, BF16), _dev(dy_np, BF16), _dev(table)
    assert _L().lib().pcd_sparse_conv_wgrad_os_splits(case.cap, 27, case.cin_pad, 16) == -(-case.cap // 1024)
    n_dev = _i32(n) if case.cap > n else None
    dw = ops.wgrad(x, case.cin, dy, None, None, 27, nbr_out=tab, n_out_dev=n_dev)
    assert dw.shape == (16, 27, case.cin)
    _judge("wgrad_os16_kernel", f"cin_pad={case.cin_pad} n={n} of {case.cap}", dw, ref, "wgrad")
    _same_bits(dw, ops.wgrad(x, case.cin, dy, None, None, 27, nbr_out=tab, n_out_dev=n_dev), "second run")
    if case.cap > n:
        host = ops.wgrad(x, case.cin, dy[:n].contiguous(), None, None, 27, nbr_out=tab[:, :n].contiguous())
        _same_bits(dw, host, "device against host count")


def test_wgrad_column_block_input(pcd_option):
    """x_block=True: x is a column block of a wider row-major matrix.  wgrad_kernel reads it through the row stride; wgrad128_kernel
    takes rows of exactly 128 channels and refuses the block (PCD_ERR_UNSUPPORTED) -- under "wg128" = 0 the generic kernel serves it."""
    ops = _ops()
    L = _L()
    pcd_option("wg_rows", R.WG_ROWS)
    for case in (R.WG_KERNEL_CASES[4], R.WG_KERNEL_CASES[11]):        # 32 x 32; 128 x 128 (wgrad128, then the generic kernel)
        d = R.wg_data(case)
        ref = R.ref_wgrad(d.x, d.dy, d.pairs, d.pair_num, case.cin)
        wide = torch.full((case.n_x, case.cin + 24), float("nan"), dtype=BF16, device=DEV)
        wide[:, 8:8 + case.cin] = _dev(d.x, BF16)
        xb = wide[:, 8:8 + case.cin]
        dy, pairs, num = _dev(d.dy, BF16), _dev(d.pairs), _dev(d.pair_num)
        K = len(case.counts)
        if case.cin == 128:
            with pytest.raises(L.PcdError, match=r"code -2"):
                ops.wgrad(xb, case.cin, dy, pairs, num, K, x_block=True)
            pcd_option("wg128", 0)
        dw = ops.wgrad(xb, case.cin, dy, pairs, num, K, x_block=True)
        _judge("wgrad_kernel", case.name + " column block", dw, ref, "wgrad")
