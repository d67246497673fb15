"""What the VectorPool tests share (test_vector_pool_cpu.py, test_gpu_vector_pool.py, tests/golden/make_golden_vector_pool.py): a
numpy restatement of the natives of pointnet2_stack/src/vector_pool_gpu.cu under the contract of include/pcd_ops.h section f6
-- f32 arithmetic in the stated order, no contraction --, the conditions the fixture g36 was drawn under, the configurations of
g36 / g37, and the bar against the reference's fp64 values (that of tests/voxel_pool_ref.py::check)."""
import json

import numpy as np

F = np.float32
CAP = 1000
MULTIPLE = 6                      # ours vs fp64 <= MULTIPLE x the deviation of the reference's own f32 run from its fp64 run

# g36: (num_grid, max_neighbour_distance, neighbor_type, nsample); the three-NN queries at 2 x the distance
OPS = [((2, 2, 2), 0.5, 0, -1), ((3, 3, 3), 0.45, 1, -1), ((1, 2, 3), 0.5, 0, 5), ((3, 3, 3), 0.45, 1, 5)]
MULTIPLIER = 2.0
OP_CHANNELS = 4
# ... and what the modules of g37 query on the same geometry (cube test; local_interpolation -1, voxel_random_choice 32)
MODULE_OPS = [((2, 2, 2), 0.5, 0, 32), ((3, 3, 3), 0.45, 0, -1), ((3, 3, 3), 0.45, 0, 32)]


def frame_ranges(cnt):
    ends = np.cumsum(np.asarray(cnt, np.int64))
    return ends - np.asarray(cnt, np.int64), ends


def frame_of_queries(new_cnt):
    return np.repeat(np.arange(len(new_cnt)), np.asarray(new_cnt, np.int64))


def within(local, r, neighbor_type):
    """the cube / ball test of vector_pool_gpu.cu:170-183 on local = support - new [K, 3] (f32) -> keep mask"""
    r = F(r)
    lx, ly, lz = local[:, 0], local[:, 1], local[:, 2]
    if neighbor_type == 1:
        return ~((lx * lx + ly * ly) + lz * lz > r * r)
    return ~((np.abs(lx) > r) | (np.abs(ly) > r) | (np.abs(lz) > r))


def neighbor_lists(support_xyz, xyz_cnt, new_xyz, new_cnt, r, nsample, neighbor_type, cap=CAP):
    """query_stacked_local_neighbor_idxs_kernel: per query the first min(cap, nsample > 0 ? nsample : cap) GLOBAL rows of its
    frame within r, ascending -> (list of int arrays, uncapped counts)"""
    support_xyz, new_xyz = np.asarray(support_xyz, F), np.asarray(new_xyz, F)
    starts, ends = frame_ranges(xyz_cnt)
    take = min(cap, nsample) if nsample > 0 else cap
    lists, full = [], np.zeros(len(new_xyz), np.int64)
    for m, b in enumerate(frame_of_queries(new_cnt)):
        rows = np.arange(starts[b], ends[b])
        hit = rows[within(support_xyz[rows] - new_xyz[m], r, neighbor_type)]
        full[m] = len(hit)
        lists.append(hit[:take])
    return lists, full


def three_nn(support_xyz, xyz_cnt, new_xyz, centers, new_cnt, r, nsample, neighbor_type):
    """pcd_vector_pool_three_nn -> idx int32 [M, G, 3], dist2 f32 [M, G, 3], neighbor_cnt int32 [M]"""
    support_xyz, centers = np.asarray(support_xyz, F), np.asarray(centers, F)
    lists, _ = neighbor_lists(support_xyz, xyz_cnt, new_xyz, new_cnt, r, nsample, neighbor_type)
    M, G = centers.shape[:2]
    idx = np.full((M, G, 3), -1, np.int32)
    dist2 = np.full((M, G, 3), np.inf, F)
    for m, rows in enumerate(lists):
        if len(rows) == 0:
            continue
        p, c = support_xyz[rows][None, :, :], centers[m][:, None, :]
        d = ((c[..., 0] - p[..., 0]) * (c[..., 0] - p[..., 0]) + (c[..., 1] - p[..., 1]) * (c[..., 1] - p[..., 1])) \
            + (c[..., 2] - p[..., 2]) * (c[..., 2] - p[..., 2])                      # [G, K] f32, left to right
        order = np.argsort(d, axis=1, kind="stable")[:, :3]                           # (d, position)
        if order.shape[1] < 3:                                                        # one / two neighbours: slot 1 again
            order = np.concatenate([order, np.repeat(order[:, :1], 3 - order.shape[1], axis=1)], axis=1)
        idx[m] = rows[order]
        dist2[m] = np.take_along_axis(d, order, axis=1)
    return idx, dist2, np.array([len(r_) for r_ in lists], np.int32)


def three_interpolate(features, idx, weight):
    """three_interpolate_kernel_stack (interpolate_gpu.cu): features [N, C], idx / weight [K, 3] -> [K, C], in the dtype given"""
    return (weight[:, 0:1] * features[idx[:, 0]] + weight[:, 1:2] * features[idx[:, 1]]) + weight[:, 2:3] * features[idx[:, 2]]


def grid_cells(local, r, num_grid):
    """cell of each local [K, 3] (f32): floorf((local_a + r) / grid_size_a) per axis, combined, then clamped; also the three
    quotients (for the fixture's distance to a cell border)"""
    r = F(r)
    q = np.stack([(local[:, a] + r) / (r * F(2) / F(num_grid[a])) for a in range(3)], axis=1)
    i = np.floor(q).astype(np.int64)
    G = num_grid[0] * num_grid[1] * num_grid[2]
    return np.clip(i[:, 0] * num_grid[1] * num_grid[2] + i[:, 1] * num_grid[2] + i[:, 2], 0, G - 1), q


def voxel_query(support_xyz, xyz_cnt, support_features, new_xyz, new_cnt, num_grid, r, nsample, neighbor_type, dtype=F):
    """pcd_vector_pool_voxel_query_forward (vector_pool_kernel_stack, pooling_type 1) -> new_features [M, G * c], new_local_xyz
    [M, 3 * G] (in `dtype`: the reference's fp64 run forms the coordinates in fp64; the decisions are taken in f32),
    point_cnt_of_grid int32 [M, G], src_row int32 [M, G]"""
    sx32, nx32 = np.asarray(support_xyz, F), np.asarray(new_xyz, F)
    feats = np.asarray(support_features, dtype)
    starts, ends = frame_ranges(xyz_cnt)
    G, c, M = num_grid[0] * num_grid[1] * num_grid[2], feats.shape[1], len(nx32)
    want = min(G, nsample) if nsample > 0 else G
    out, loc = np.zeros((M, G, c), dtype), np.zeros((M, G, 3), dtype)
    cnt, src = np.zeros((M, G), np.int32), np.full((M, G), -1, np.int32)
    for m, b in enumerate(frame_of_queries(new_cnt)):
        rows = np.arange(starts[b], ends[b])
        local = sx32[rows] - nx32[m]
        keep = within(local, r, neighbor_type)
        rows, local = rows[keep], local[keep]
        if len(rows) == 0:
            continue
        cells, _ = grid_cells(local, r, num_grid)
        uniq, first = np.unique(cells, return_index=True)                             # first hit of each cell ...
        first = np.sort(first)[:want]                                                 # ... in row order, until `want` are filled
        g = cells[first]
        src[m, g], cnt[m, g] = rows[first], 1
        out[m, g] = feats[rows[first]]
        loc[m, g] = np.asarray(support_xyz, dtype)[rows[first]] - np.asarray(new_xyz, dtype)[m]
    return out.reshape(M, G * c), loc.reshape(M, G * 3), cnt, src


def voxel_query_grad(grad_new_features, src_row, N):
    """pcd_vector_pool_voxel_query_backward in fp64: grad_support[src_row[m, g]] += grad_new_features[m, g, :]"""
    M, G = src_row.shape
    g = np.asarray(grad_new_features, np.float64).reshape(M, G, -1)
    out = np.zeros((N, g.shape[2]), np.float64)
    has = src_row >= 0
    np.add.at(out, src_row[has], g[has])
    return out


def dense_offsets(r, num_grid):
    """VectorPoolAggregationModule.get_dense_voxels_by_center's offsets [G, 3] as torch.arange forms them on the host"""
    import torch
    grids = [torch.arange(-r + r / n, r - r / n + 1e-5, 2 * r / n) for n in num_grid]
    return torch.stack([t.reshape(-1) for t in torch.meshgrid(*grids, indexing="ij")], dim=1).numpy().astype(F)


# ---------------------------------------------------------------------------------------------------------------------
def fixture_violations(support_xyz, xyz_cnt, new_xyz, new_cnt, ops=tuple(OPS + MODULE_OPS), rel=1e-5, tie=1e-6):
    """the margins g36 was drawn under -> set of support rows behind a violation (empty: all hold).  Every |local_a| and every
    squared distance more than `rel` (relative to the threshold) from the query distances r and MULTIPLIER * r; every
    (local_a + r) / grid_size_a of a hit more than `rel` from an integer; per (m, g) the four smallest distances of the list
    pairwise more than `tie` relative apart."""
    sx, nx = np.asarray(support_xyz, F), np.asarray(new_xyz, F)
    starts, ends = frame_ranges(xyz_cnt)
    bad = set()
    frames = frame_of_queries(new_cnt)
    for num_grid, r, ntype, nsample in ops:
        offsets = dense_offsets(r, num_grid)
        for m, b in enumerate(frames):
            rows = np.arange(starts[b], ends[b])
            local = (sx[rows] - nx[m]).astype(np.float64)
            for dist in (r, MULTIPLIER * r):
                near = np.abs(np.abs(local) - dist) <= rel * dist
                d2 = (local * local).sum(1)
                near_ball = np.abs(d2 - dist * dist) <= rel * dist * dist
                bad.update(rows[near.any(1) | near_ball].tolist())
            hit = within(sx[rows] - nx[m], r, ntype)
            if hit.any():
                _, q = grid_cells((sx[rows] - nx[m])[hit], r, num_grid)
                bad.update(rows[hit][(np.abs(q - np.round(q)) <= rel).any(1)].tolist())
            lst = rows[within(sx[rows] - nx[m], F(MULTIPLIER * r), ntype)][:(min(CAP, nsample) if nsample > 0 else CAP)]
            if len(lst) >= 2:
                c = (nx[m] + offsets).astype(np.float64)
                d = ((c[:, None, :] - sx[lst][None, :, :].astype(np.float64)) ** 2).sum(2)         # [G, K]
                order = np.argsort(d, axis=1, kind="stable")[:, :4]
                top = np.take_along_axis(d, order, axis=1)
                close = (top[:, 1:] - top[:, :-1]) <= tie * top[:, 1:]
                for g, k in zip(*np.nonzero(close)):
                    bad.add(int(lst[order[g, k + 1]]))
    return bad


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev(a, ref64):
    """largest deviation relative to the largest fp64 value"""
    return float(np.abs(np.asarray(a, np.float64) - ref64).max() / max(np.abs(ref64).max(), 1e-30))


def check(name, ours, g, key):
    """ours against g[key + '_f64'] under the bar the stored f32 run sets (tests/voxel_pool_ref.py::check)"""
    e, r = dev(ours, g[key + "_f64"]), dev(g[key + "_f32"], g[key + "_f64"])
    bar = MULTIPLE * r
    print(f"[{name}] ours vs fp64 {e:.2e}, the reference's f32 {r:.2e}, bar {bar:.2e}")
    assert e <= bar, (name, e, r, bar)


def module_cfg(g, kind):
    return json.loads(bytes(g[f"{kind}_cfg_json"]).decode())


def module_cfgs():
    """the two configurations of g37 (tests/golden/make_golden_vector_pool.py): -> {kind: (input channels, config)}"""
    groups = dict(GROUP_CFG_0=dict(NUM_LOCAL_VOXEL=[2, 2, 2], MAX_NEIGHBOR_DISTANCE=0.5, NEIGHBOR_NSAMPLE=-1, POST_MLPS=[8, 8]),
                  GROUP_CFG_1=dict(NUM_LOCAL_VOXEL=[3, 3, 3], MAX_NEIGHBOR_DISTANCE=0.45, NEIGHBOR_NSAMPLE=-1, POST_MLPS=[8, 6]))
    interp = dict(NAME="VectorPoolAggregationModuleMSG", NUM_GROUPS=2, LOCAL_AGGREGATION_TYPE="local_interpolation",
                  NUM_REDUCED_CHANNELS=3, NUM_CHANNELS_OF_LOCAL_AGGREGATION=4, MSG_POST_MLPS=[10], **json.loads(json.dumps(groups)))
    choice = dict(NAME="VectorPoolAggregationModuleMSG", NUM_GROUPS=2, LOCAL_AGGREGATION_TYPE="voxel_random_choice",
                  NUM_REDUCED_CHANNELS=4, NUM_CHANNELS_OF_LOCAL_AGGREGATION=4, MSG_POST_MLPS=[10], **json.loads(json.dumps(groups)))
    for k in ("GROUP_CFG_0", "GROUP_CFG_1"):
        choice[k]["NEIGHBOR_NSAMPLE"] = 32
    return {"local_interpolation": (6, interp), "voxel_random_choice": (4, choice)}
