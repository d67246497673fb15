"""GPU: Voxel R-CNN's RoI-grid pooling (com_amd/csrc/voxelpool.hip) -- the voxel -> row map, the cooperative query against
the oracle, NeighborVoxelSAModuleMSG against the fp64 values of the reference's own class (fixture g34,
tests/golden/make_golden_voxel_rcnn.py) under the bar of tests/voxel_pool_ref.py, the pooling kernels at channel counts the
fixture does not have, reproducibility and the memory the fused form keeps."""
import types

import numpy as np
import pytest
import torch

from com_amd import pointnet2_stack as P
from com_amd.hotpath.pvrcnn_stage2 import generate_voxel2pinds
from oracle import oracle as O
from tests.voxel_pool_ref import CHANNELS, LEVELS, cfg_of, check, pool_restated
from tests.voxel_pool_ref import cu as _cu

pytestmark = pytest.mark.gpu


def test_voxel2pinds_scatter_honours_num_rows_and_clear_restores(golden):
    r = np.random.default_rng(1)
    B, Z, Y, X, N, rows = 3, 5, 9, 11, 300, 217
    cells = r.permutation(B * Z * Y * X)[:N]
    ind = np.stack(np.unravel_index(cells, (B, Z, Y, X)), 1).astype(np.int32)
    want = np.full((B, Z, Y, X), -1, np.int32)
    want[tuple(ind[:rows].T)] = np.arange(rows, dtype=np.int32)
    sp = types.SimpleNamespace(indices=_cu(ind), spatial_shape=[Z, Y, X], batch_size=B,
                               num_rows=torch.tensor([rows], dtype=torch.int32, device="cuda"))
    v2p = generate_voxel2pinds(sp)
    assert v2p.dtype == torch.int32 and np.array_equal(v2p.cpu().numpy(), want)
    P.voxel2pinds_clear(sp.indices, v2p, sp.num_rows)
    assert bool((v2p == -1).all())
    sp.num_rows = None
    full = generate_voxel2pinds(sp, out=v2p)
    want[tuple(ind.T)] = np.arange(N, dtype=np.int32)
    assert full is v2p and np.array_equal(full.cpu().numpy(), want)
    ind_bad = ind.copy()
    ind_bad[0] = (B, 0, 0, 0)                                                 # a row outside the map is skipped, not written
    P.voxel2pinds_clear(_cu(ind_bad), v2p)
    want[:] = -1
    want[tuple(ind[0])] = 0
    assert np.array_equal(v2p.cpu().numpy(), want)


def _moments(xyz, new_xyz, idx, empty):
    r = (xyz[idx] - new_xyz[:, None, :]).astype(np.float64)                   # formed in f32, as the kernel forms it
    r[empty] = 0
    r = r.reshape(-1, 3)
    return np.array([r[:, 0].sum(), r[:, 1].sum(), r[:, 2].sum(), (r[:, 0] * r[:, 0]).sum(), (r[:, 0] * r[:, 1]).sum(),
                     (r[:, 0] * r[:, 2]).sum(), (r[:, 1] * r[:, 1]).sum(), (r[:, 1] * r[:, 2]).sum(), (r[:, 2] * r[:, 2]).sum()])


def _check_query(rng, radius, ns, xyz, new_xyz, coords_zyx, v2p, want_idx, want_empty):
    idx, cnt, mom = P.voxel_pool_query(rng, radius, ns, _cu(xyz), _cu(new_xyz), _cu(coords_zyx), _cu(v2p))
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    assert idx.dtype == np.int32 and np.array_equal(idx, want_idx)
    assert np.array_equal(cnt == 0, want_empty)
    distinct = np.where(want_empty, 0, 1 + (want_idx[:, 1:] != want_idx[:, :1]).sum(1))
    assert np.array_equal(cnt, distinct)
    want = _moments(xyz, new_xyz, want_idx, want_empty)
    assert np.abs(mom.cpu().numpy() - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0) * len(want_idx)
    return cnt


@pytest.mark.parametrize("src", LEVELS)
def test_query_is_bit_exact_on_the_fixture(golden, src):
    g = golden("g34_voxel_pool")
    lc = cfg_of(g)["ROI_GRID_POOL"]["POOL_LAYERS"][src]
    coords = np.ascontiguousarray(g[f"{src}_new_coords"][:, [0, 3, 2, 1]])
    for s, (rng, radius, ns) in enumerate(zip(lc["QUERY_RANGES"], lc["POOL_RADIUS"], lc["NSAMPLE"])):
        cnt = _check_query(rng, radius, ns, g[f"{src}_xyz"], g["new_xyz"], coords, g[f"{src}_v2p"], g[f"{src}_idx{s}"],
                           g[f"{src}_empty{s}"])
        assert (cnt == 0).any() and (cnt == ns).any() and (cnt > 0).any()


@pytest.mark.parametrize("M", [1, 37])
def test_query_random_case_with_out_of_grid_coordinates(M):
    r = np.random.default_rng(100 + M)
    B, Z, Y, X = 2, 4, 7, 9
    keep = r.random((B, Z, Y, X)) < 0.5
    ind = np.stack(np.nonzero(keep), 1).astype(np.int32)
    ind = ind[r.permutation(len(ind))]
    v2p = np.full((B, Z, Y, X), -1, np.int32)
    v2p[tuple(ind.T)] = np.arange(len(ind), dtype=np.int32)
    xyz = ((ind[:, [3, 2, 1]] + 0.5) * np.float32(0.5)).astype(np.float32)
    coords = np.stack([r.integers(0, B, M), r.integers(-3, Z + 3, M), r.integers(-3, Y + 3, M), r.integers(-3, X + 3, M)], 1).astype(np.int32)
    coords[0, 1:] = (-2, Y + 1, X // 2)                                       # outside in z and y at once
    new_xyz = ((coords[:, [3, 2, 1]] + r.random((M, 3))) * 0.5).astype(np.float32)
    for rng, radius, ns in (([2, 3, 1], 0.83, 7), ([4, 4, 4], 1.37, 16), ([0, 0, 0], 0.4, 3)):
        want_idx, want_empty = O.voxel_query_stack(rng, radius, ns, xyz, new_xyz, coords, v2p)
        _check_query(rng, radius, ns, xyz, new_xyz, coords, v2p, want_idx, want_empty)


def _layer(g, level, src):
    lc = cfg_of(g)["ROI_GRID_POOL"]["POOL_LAYERS"][src]
    layer = P.NeighborVoxelSAModuleMSG(query_ranges=lc["QUERY_RANGES"], nsamples=lc["NSAMPLE"], radii=lc["POOL_RADIUS"],
                                       mlps=[[CHANNELS[src]] + m for m in lc["MLPS"]], pool_method="max_pool")
    pre = f"state.{level}."
    layer.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pre)}, strict=True)
    return layer.cuda()


def _forward(layer, g, src, feats):
    return layer(xyz=_cu(g[f"{src}_xyz"]), xyz_batch_cnt=None, new_xyz=_cu(g["new_xyz"]), new_xyz_batch_cnt=None,
                 new_coords=_cu(g[f"{src}_new_coords"]), features=feats, voxel2point_indices=_cu(g[f"{src}_v2p"]))


@pytest.mark.parametrize("level, src", list(enumerate(LEVELS)))
def test_module_meets_the_fp64_fixture(golden, level, src):
    """training output, the gradients of sum(out * probe) with respect to the features and every parameter, the running
    statistics after the step, and the eval output with those statistics"""
    g = golden("g34_voxel_pool")
    layer = _layer(g, level, src).train()
    feats = _cu(g[f"{src}_features"]).requires_grad_(True)
    y = _forward(layer, g, src, feats)
    assert tuple(y.shape) == (324, 16) and y.dtype == torch.float32
    (y * _cu(g[f"{src}_probe"])).sum().backward()
    check(f"{src} train", y.detach().cpu().numpy(), g, f"{src}_train")
    check(f"{src} d features", feats.grad.cpu().numpy(), g, f"{src}_dfeatures")
    for name, p in layer.named_parameters():
        check(f"{src} d {name}", p.grad.cpu().numpy(), g, f"{src}_grad.{name}")
    for name, b in layer.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(g[f"{src}_after.{name}_f64"]) == 1
        else:
            check(f"{src} {name}", b.cpu().numpy(), g, f"{src}_after.{name}")
    layer.eval()
    with torch.no_grad():
        check(f"{src} eval", _forward(layer, g, src, feats).cpu().numpy(), g, f"{src}_eval")


@pytest.mark.parametrize("C, ns", [(40, 5), (128, 16), (33, 1)])
def test_pool_kernels_beyond_32_channels(C, ns):
    """voxel_pool (forward, winner, backward) where the kernels run 64 lanes along c, against the fp64 restatement from the
    same f32 inputs.  Bars from the arithmetic: an output is six f32 roundings of partial sums no larger than the sum of the
    absolute terms (8 ulps of it asked); a gradient is an f32 sum of at most M terms, so M ulps of the sum of its absolute
    terms.  The gradient probe is zero where the winner or its sign is within 1e-4 of a tie, which f32 may break either way."""
    r = np.random.default_rng(C)
    B, Z, Y, X, M = 2, 4, 9, 8, 203
    ind = np.stack(np.nonzero(r.random((B, Z, Y, X)) < 0.4), 1).astype(np.int32)
    ind = ind[r.permutation(len(ind))]
    N = len(ind)
    v2p = np.full((B, Z, Y, X), -1, np.int32)
    v2p[tuple(ind.T)] = np.arange(N, dtype=np.int32)
    xyz = ((ind[:, [3, 2, 1]] + 0.5) * np.float32(0.5)).astype(np.float32)
    coords = np.stack([r.integers(0, B, M), r.integers(-3, Z + 3, M), r.integers(-3, Y + 3, M), r.integers(-3, X + 3, M)], 1).astype(np.int32)
    new_xyz = ((coords[:, [3, 2, 1]] + r.random((M, 3))) * 0.5).astype(np.float32)
    fin, A, b = (torch.from_numpy(r.standard_normal(shape).astype(np.float32)) for shape in ((N, C), (C, 3), (C,)))
    idx, cnt, _ = P.voxel_pool_query([2, 3, 3], 1.3, ns, _cu(xyz), _cu(new_xyz), _cu(coords), _cu(v2p))
    assert bool((cnt == 0).any()) and bool((cnt == ns).any())
    g = torch.from_numpy(r.standard_normal((M, C)).astype(np.float32))
    ref = pool_restated(fin, A, b, torch.from_numpy(xyz), torch.from_numpy(new_xyz), idx.cpu(), cnt.cpu(), g)
    clear = (ref["out"] == 0) | ((ref["gap"] > 1e-4) & (ref["out"] > 1e-4))
    g = g * clear
    ref = pool_restated(fin, A, b, torch.from_numpy(xyz), torch.from_numpy(new_xyz), idx.cpu(), cnt.cpu(), g)
    leaves = [t.cuda().requires_grad_(True) for t in (fin, A, b)]
    out = P.voxel_pool(*leaves, _cu(xyz), _cu(new_xyz), idx, cnt)
    assert tuple(out.shape) == (M, C)
    out.backward(g.cuda())
    ulp = 2.0 ** -24
    err = (out.detach().cpu().double() - ref["out"]).abs()
    print(f"[C = {C}] out: largest error / bar {float((err / (8 * ulp * ref['mag_out'])).max()):.2f}")
    assert bool((err <= 8 * ulp * ref["mag_out"]).all())
    for name, leaf in zip(("d_fin", "dA", "db"), leaves):
        want, mag = ref[name], ref["mag_" + name.replace("d_", "")]
        err = (leaf.grad.cpu().double() - want).abs()
        bar = M * ulp * mag
        print(f"[C = {C}] {name}: largest error {float(err.max()):.2e}, largest bar {float(bar.max()):.2e}")
        assert bool((err <= bar).all()), name
    assert bool((ref["d_fin"] != 0).any()) and bool(clear.float().mean() > 0.9)


def test_two_forward_runs_are_bit_identical(golden):
    g = golden("g34_voxel_pool")
    outs = []
    for _ in range(2):
        layer = _layer(g, 0, "x_conv1").train()
        feats = _cu(g["x_conv1_features"]).requires_grad_(True)
        y = _forward(layer, g, "x_conv1", feats)
        outs.append((y.detach().clone(), layer.mlps_pos[0][1].running_var.clone(), layer.mlps_pos[1][1].running_mean.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_no_grouped_tensor_is_kept():
    """M = 4096 queries, C = 32, nsample = 16: forward + backward of one scale allocate less than ONE [M, C, nsample] f32
    tensor beyond what was live before (the composed form keeps several)"""
    torch.manual_seed(3)
    B, Z, Y, X, M, C, ns = 2, 8, 40, 40, 4096, 32, 16
    keep = torch.rand(B, Z, Y, X, device="cuda") < 0.3
    ind = keep.nonzero().int()
    sp = types.SimpleNamespace(indices=ind, spatial_shape=[Z, Y, X], batch_size=B, num_rows=None)
    v2p = generate_voxel2pinds(sp)
    xyz = (ind[:, [3, 2, 1]].float() + 0.5) * 0.5
    coords = torch.stack([torch.randint(0, B, (M,)), torch.randint(0, X, (M,)), torch.randint(0, Y, (M,)), torch.randint(0, Z, (M,))],
                         1).int().cuda()
    new_xyz = (coords[:, 1:4].float() + torch.rand(M, 3, device="cuda")) * 0.5
    layer = P.NeighborVoxelSAModuleMSG(query_ranges=[[4, 4, 4]], radii=[1.2], nsamples=[ns], mlps=[[16, C, 32]]).cuda().train()
    feats = torch.randn(ind.shape[0], 16, device="cuda", requires_grad=True)

    def step():
        y = layer(xyz, None, new_xyz, None, coords, feats, v2p)
        y.square().mean().backward()
        return y
    step()                                                                     # warm-up: library workspaces
    layer.zero_grad(), feats.grad.zero_()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y = step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"[memory] peak rise across forward + backward {rise / 2 ** 20:.2f} MiB; one [M, C, nsample] f32 tensor "
          f"{M * C * ns * 4 / 2 ** 20:.2f} MiB")
    assert torch.isfinite(y).all() and rise < M * C * ns * 4
