"""tests/sparse_conv_ref.py checked without a GPU: the float64 reference agrees with two independent computations (the C oracle,
and the torch conv3d fp64 arrays of fixture g3_conv), and every edge case tests/test_gpu_sparse_conv_edges.py runs can tell a
wrong kernel from a right one -- a float32 evaluation of the same sums stays inside the tolerance the device test applies, each
of a list of wrong results lands outside it."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import sparse_conv_ref as R
from tests.test_oracle_golden import GEOMS


def _rulebook(g, name):
    geo = GEOMS[name]
    idx, shape = g["indices"], g["spatial_shape"]
    return O.rulebook_subm(idx, shape, geo["k"], 1) if geo["subm"] else O.rulebook_conv(idx, shape, geo["k"], geo["s"], geo["p"], 1)


def _close32(got, ref, what):
    """float32 rounding of sums of a few thousand terms of either sign: 1e-5 of the largest magnitude (the oracle accumulates in
    float32 in pair order; measured: below 2e-6)"""
    err = np.abs(np.asarray(got, np.float64) - ref).max()
    assert err <= 1e-5 * np.abs(ref).max(), (what, err, np.abs(ref).max())


# ---- agreement with independent computations ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["subm_k3", "conv_k3_s2_p1"])
def test_reference_agrees_with_the_oracle(golden, name):
    g = golden("g3_conv")
    rb = _rulebook(g, name)
    rng = np.random.default_rng(5)
    K, cin, cout = rb["K"], 16, 32
    x = R.normal_bf16(rng, rb["n_in"], cin)
    w = R.normal_bf16(rng, K, cin, cout, scale=0.1)
    bias = rng.standard_normal(cout).astype(np.float32)
    gy = R.normal_bf16(rng, rb["n_out"], cout)
    _close32(O.conv_fwd(x, w, bias, rb), R.ref_gather_gemm(x, w, bias, rb["nbr_out"], False), "forward")
    dx_o, dw_o, _ = O.conv_bwd(x, w, gy, rb)
    wt = np.ascontiguousarray(np.transpose(w, (0, 2, 1)))                  # W[k]^T: cout -> cin
    _close32(dx_o, R.ref_gather_gemm(gy, wt, None, rb["nbr_in"], False), "dgrad over nbr_in")
    if GEOMS[name]["subm"]:                                                 # the flipped-offset rule
        _close32(dx_o, R.ref_gather_gemm(gy, wt, None, rb["nbr_out"], True), "dgrad, flipped offsets")
    dw = R.ref_wgrad(x, gy, rb["pairs"], rb["pair_num"])                   # [cout, K, cin]
    _close32(np.transpose(dw_o, (2, 0, 1)), dw, "wgrad")
    pairs, num = R.pairs_of_table(rb["nbr_out"], rb["n_out"])
    assert np.array_equal(num, rb["pair_num"])
    assert np.array_equal(dw, R.ref_wgrad(x, gy, pairs, num))
    _close32(R.ref_wgrad_table(x, gy, rb["nbr_out"], rb["n_out"], cin), dw, "wgrad over the table")


@pytest.mark.parametrize("name", list(GEOMS))
def test_reference_agrees_with_dense_conv3d_fixture(golden, name):
    """the *_bf16in_* arrays are float32 copies of torch conv3d results computed in fp64: agreement to float32 rounding"""
    g = golden("g3_conv")
    rb = _rulebook(g, name)
    pre = f"{name}_bf16in_"
    x, w, gy = g["x_bf16in"], g[pre + "w"], g[pre + "gy"]
    for got, key in ((R.ref_gather_gemm(x, w, None, rb["nbr_out"], False), "y"),
                     (R.ref_gather_gemm(gy, np.transpose(w, (0, 2, 1)), None, rb["nbr_in"], False), "dx"),
                     (np.transpose(R.ref_wgrad(x, gy, rb["pairs"], rb["pair_num"]), (1, 2, 0)), "dw")):
        ref = g[pre + key].astype(np.float64)
        assert np.abs(got - ref).max() <= 2.0 ** -23 * np.abs(ref).max(), (name, key)


# ---- sensitivity of the gather-GEMM cases -----------------------------------------------------------------------------------------
def _gg_all_cases():
    out = {}
    for inst in R.GG_INSTS:
        tiles = {inst.tile} if inst.wide else {R.gg_tile(inst, False), R.gg_tile(inst, True)}
        for t in sorted(tiles):
            out.update({f"{inst.name} n={c.n_out}": c for c in R.gg_cases(inst, t)})
    for inst in R.DEVCOUNT_INSTS:
        out.update({f"{inst.name} n_dev={nd}": c for nd, c in R.devcount_cases(inst) if nd > 0})
    for inst, mode in R.BN_CASES:
        out.update({f"{inst.name} mode {mode} {'device' if dev else 'host'} count": R.bn_case(inst, mode, dev) for dev in (False, True)})
    return [pytest.param(c, id=name) for name, c in out.items()]


def _outside(mut, ref, kinds, what):
    for kind in kinds:
        got = R.bf16_round(mut) if kind == "bf16" else mut
        assert R.excess(got, ref, kind) > 1.0, f"{what}: not told apart at the {kind} tolerance"


def _check_gg_sensitivity(case, d, rows=None):
    """rows: judge these output rows only (the 45 k-row case: every mutation below changes rows inside them)"""
    i = case.inst
    nbr = d.nbr if rows is None else np.ascontiguousarray(d.nbr[:, rows])
    add = d.addend if d.addend is None or rows is None else d.addend[rows]
    ref = R.ref_gather_gemm(d.x, d.w, d.bias, nbr, i.flip, add)
    assert np.abs(ref).max() > 0
    f32 = R.f32_gather_gemm(d.x, d.w, d.bias, nbr, i.flip, add)
    assert R.excess(f32, ref, "f32") <= 1.0 and R.excess(R.bf16_round(f32), ref, "bf16") <= 1.0
    kinds = ("f32", "bf16")
    n_in, K = d.x.shape[0], i.kvol
    # one pair dropped (the first present entry of the middle row)
    m = nbr.copy()
    ks, os_ = np.nonzero((m >= 0) & (m < n_in))
    pick = np.argsort(os_, kind="stable")[len(os_) // 2]
    m[ks[pick], os_[pick]] = -1
    _outside(R.ref_gather_gemm(d.x, d.w, d.bias, m, i.flip, add), ref, kinds, "one pair dropped")
    # the last row of the (partial) last tile dropped: its gathers contribute nothing
    m = nbr.copy()
    assert (m[:, -1] >= 0).any(), "the last row needs a neighbour"
    m[:, -1] = -1
    _outside(R.ref_gather_gemm(d.x, d.w, d.bias, m, i.flip, add), ref, kinds, "last row dropped")
    # k and K - 1 - k swapped
    if i.flip:
        _outside(R.ref_gather_gemm(d.x, d.w, d.bias, nbr, False, add), ref, kinds, "offsets not flipped")
    # the last input row read as zeros
    assert (nbr == n_in - 1).any(), "the table must name the last input row"
    xz = d.x.copy()
    xz[n_in - 1] = 0
    _outside(R.ref_gather_gemm(xz, d.w, d.bias, nbr, i.flip, add), ref, kinds, "last input row read as zero")


@pytest.mark.parametrize("case", _gg_all_cases())
def test_gather_gemm_cases_tell_mutations_apart(case):
    _check_gg_sensitivity(case, R.gg_data(case))


def test_gather_gemm_45k_case_tells_mutations_apart():
    idx, batch, shape = R.random_cells(*R.GRID_45K)
    table = O.rulebook_subm(idx, shape)["nbr_out"]
    assert table.shape == (27, 45000) and 45000 % 192 != 0          # a partial last 192-row tile
    case = R.CASE_45K
    d = R.gg_data(case, table)
    rows = np.r_[0:192, 45000 - 72:45000]                            # the first tile and the partial last one
    assert d.nbr[13, -1] == case.n_in - 1                            # (the centre offset of a SubM table: the row itself)
    _check_gg_sensitivity(case, d, rows)


@pytest.mark.parametrize("gname,idx,batch,shape", [pytest.param(*g, id=g[0]) for g in R.class_grids()])
def test_class_kernel_cases_tell_mutations_apart(gname, idx, batch, shape):
    """the data gradient over nbr_in of the strided conv on the three edge grids (tables from the CPU oracle; the device test checks that
    the device rulebook is the same table)"""
    nbr_in, nbr_out = R.oracle_strided(idx, shape)
    assert nbr_in.shape[1] == idx.shape[0]
    if gname == "one parity class":
        assert len(np.unique(idx[:, 1:] % 2, axis=0)) == 1
    for c_dy, c_in, seed in R.CLASS_WIDTHS:
        case = R.class_case(c_dy, c_in, seed, nbr_in.shape[1], nbr_out.shape[1])
        _check_gg_sensitivity(case, R.gg_data(case, nbr_in))


def test_packed_table_cases_tell_mutations_apart():
    idx, _, shape = R.random_cells(*R.SMALL_GRID)
    assert np.array_equal(idx, idx[R.yxz_order(idx)])                # the rows come ascending in (b, y, x, z)
    nbr_in, nbr_out = R.oracle_strided(idx, shape, yxz=True)
    for cin, cout, seed in R.PACKED_WIDTHS:
        case = R.packed_case(cin, cout, seed, nbr_in.shape[1], nbr_out.shape[1])
        _check_gg_sensitivity(case, R.gg_data(case, nbr_out))


def test_edge_table_properties():
    t = R.gg_table(193, 230, 27, 196, "edges", 3)
    live = t[:, :193]
    assert t.dtype == np.int32 and live.min() >= -1 and live.max() == 229
    assert (live[:, 1] == -1).all() and (live[1] == -1).all()
    assert (live[2, 16:47] == -1).all() and live[2, 47] >= 0 and (live[:, -1] >= 0).any()
    assert ((t[:, 193:] < -1) | (t[:, 193:] >= 230)).all()          # garbage behind the live columns
    full = R.gg_table(64, 32, 3, 64, "full", 4)
    assert full.min() >= 0 and full.max() == 31


# ---- sensitivity of the weight-gradient cases --------------------------------------------------------------------------------------
def _check_wg_sensitivity(case, splits=False):
    d = R.wg_data(case)
    K = len(case.counts)
    for k in range(K):                                              # the builders' guarantee: ascending, distinct, in range
        p = d.pair_num[k]
        assert np.all(np.diff(d.pairs[k, 0, :p]) > 0) and np.all(d.pairs[k, :, p:] == -1)
        live = case.n_x if case.n_x_dev is None else case.n_x_dev
        assert p == 0 or (0 <= d.pairs[k, 0, 0] and d.pairs[k, 0, p - 1] < live)
        assert p == 0 or (0 <= d.pairs[k, 1, :p].min() and d.pairs[k, 1, :p].max() < case.n_dy)
    ref = R.ref_wgrad(d.x, d.dy, d.pairs, d.pair_num, case.cin)
    assert ref.shape == (case.cout, K, case.cin)
    assert R.excess(R.f32_wgrad(d.x, d.dy, d.pairs, d.pair_num, case.cin), ref, "wgrad") <= 1.0
    kmax = int(np.argmax(case.counts))
    p = int(d.pair_num[kmax])
    # one pair dropped (the middle one of the longest list); the last pair of a partial 32-pair step dropped
    for what, drop in (("one pair dropped", p // 2), ("last pair dropped", p - 1)):
        m, num = d.pairs.copy(), d.pair_num.copy()
        m[kmax, :, drop:p - 1] = m[kmax, :, drop + 1:p]
        m[kmax, :, p - 1] = -1
        num[kmax] -= 1
        assert R.excess(R.ref_wgrad(d.x, d.dy, m, num, case.cin), ref, "wgrad") > 1.0, what
    # the last input row a pair names read as zeros
    last = int(d.pairs[:, 0].max())
    xz = d.x.copy()
    xz[last] = 0
    assert R.excess(R.ref_wgrad(xz, d.dy, d.pairs, d.pair_num, case.cin), ref, "wgrad") > 1.0, "last input row read as zero"
    if splits:
        live = case.n_x if case.n_x_dev is None else case.n_x_dev
        s, _ = R.split_plan(case.n_x, case.pmax, case.cin, case.cout, R.WG_ROWS)
        per = -(-live // s)
        slabs = [R.split_slab(d.x, d.dy, d.pairs, d.pair_num, q * per, (q + 1) * per, case.cin) for q in range(s)]
        assert R.excess(sum(slabs), ref, "wgrad") <= 1e-6             # the splits partition the pairs
        return s, slabs, ref
    return None


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.WG_KERNEL_CASES + R.WG_SPLIT_CASES + R.WG128_CASES])
def test_wgrad_cases_tell_mutations_apart(case):
    if len(case.counts) == 1 and case.counts[0] == 1:                # a single pair: dropping it leaves zeros
        d = R.wg_data(case)
        ref = R.ref_wgrad(d.x, d.dy, d.pairs, d.pair_num, case.cin)
        assert np.abs(ref).max() > 0 and R.excess(np.zeros_like(ref), ref, "wgrad") > 1.0
        return
    _check_wg_sensitivity(case)


def test_wgrad_split_cases_cover_the_search_and_the_empty_slabs():
    assert [R.split_plan(c.n_x, c.pmax, c.cin, c.cout, R.WG_ROWS) for c in R.WG_SPLIT_CASES] == \
        [(2, 129), (4, 256), (11, 228), (6, 250), (8, 250)]
    assert all(R.split_plan(c.n_x, c.pmax, c.cin, c.cout, R.WG_ROWS)[0] in (2, 3) for c in R.WG_KERNEL_CASES)
    for c in R.WG_SPLIT_CASES[1:4]:
        assert {0, 1, 32, 33, 1024}.issubset(c.counts) and (1025 in c.counts or 1000 in c.counts)
    assert 1025 in R.WG_SPLIT_CASES[2].counts and 1025 in R.WG_SPLIT_CASES[3].counts
    # every input row inside one split: an empty split's slab replaced by the previous split's is told apart
    case = R.WG_SPLIT_CASES[4]
    s, slabs, ref = _check_wg_sensitivity(case, splits=True)
    empty = [q for q in range(s) if not np.any(slabs[q])]
    assert empty == [0, 1, 3, 4, 5, 6, 7]
    assert R.excess(ref + slabs[2], ref, "wgrad") > 1.0              # split 3 hands back split 2's slab
    # ... and in a case with pairs in every split, a slab counted twice in place of its neighbour's
    for case in R.WG_SPLIT_CASES[:4]:
        s, slabs, ref = _check_wg_sensitivity(case, splits=True)
        assert all(np.any(sl) for sl in slabs)
        assert R.excess(ref - slabs[1] + slabs[0], ref, "wgrad") > 1.0


@pytest.mark.parametrize("case", [pytest.param(c, id=f"cin_pad={c.cin_pad} n={c.n_out}") for c in R.OS_CASES])
def test_output_stationary_cases_tell_mutations_apart(case):
    x, dy, table = R.os_data(case)
    n = case.n_out
    ref = R.ref_wgrad_table(x, dy, table, n, case.cin)
    assert np.abs(ref).max() > 0
    assert R.excess(R.ref_wgrad_table(x, dy, table, n, case.cin, np.float32), ref, "wgrad") <= 1.0
    m = table.copy()
    k, o = np.argwhere(m[:, :n] >= 0)[np.count_nonzero(m[:, :n] >= 0) // 2]
    m[k, o] = -1
    assert R.excess(R.ref_wgrad_table(x, dy, m, n, case.cin), ref, "wgrad") > 1.0, "one pair dropped"
    m = table.copy()
    m[:, n - 1] = -1
    assert R.excess(R.ref_wgrad_table(x, dy, m, n, case.cin), ref, "wgrad") > 1.0, "last row dropped"
    xz = x.copy()
    xz[case.n_in - 1] = 0
    assert R.excess(R.ref_wgrad_table(xz, dy, table, n, case.cin), ref, "wgrad") > 1.0, "last input row read as zero"
