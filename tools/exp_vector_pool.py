#!/usr/bin/env python3
"""Time PV-RCNN++'s VectorPool aggregation (com_amd/csrc/vectorpool.hip) at the sizes of
tools/cfgs/waymo_models/pv_rcnn_plusplus.yaml: B = 4 frames, 4096 keypoints per frame, the three SA_LAYER sources (raw points,
x_conv3, x_conv4) with their channel counts, and 128 RoIs x 6^3 grid points per frame for the RoI-grid pooling.

Per row: one op (or one full module, forward + backward) captured into a graph and replayed; the figure is the median time of
REPEATS windows of REPLAYS replays each (device events around a window).  Point tests per second = queries x rows of the
query's frame over the time (an upper count: a scan that reaches its cap leaves early); bytes = what the op must read and
write once (inputs + outputs, from the shapes), against the HBM peak of 8 TB/s.

Synthetic geometry from a seed (uniform points in the Waymo range scaled so that a query sees tens to hundreds of rows): the
times depend on the density, which is printed with them.  Needs the GPU; there is no CPU path.

  python tools/exp_vector_pool.py [--out profiles/vector_pool.json] [--small]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from com_amd import pointnet2_stack as P  # noqa: E402

HBM_PEAK = 8.0e12
REPEATS, REPLAYS = 7, 5

GROUPS = lambda r0, r1, n, post: dict(  # noqa: E731
    GROUP_CFG_0=dict(NUM_LOCAL_VOXEL=[n, n, n] if r0 >= 0.4 else [2, 2, 2], MAX_NEIGHBOR_DISTANCE=r0, NEIGHBOR_NSAMPLE=-1, POST_MLPS=post),
    GROUP_CFG_1=dict(NUM_LOCAL_VOXEL=[n, n, n], MAX_NEIGHBOR_DISTANCE=r1, NEIGHBOR_NSAMPLE=-1, POST_MLPS=post))
SOURCES = {  # pv_rcnn_plusplus.yaml:84-151: (support rows per frame, input channels, config)
    'raw_points': (40000, 2, dict(NAME='VectorPoolAggregationModuleMSG', NUM_GROUPS=2, LOCAL_AGGREGATION_TYPE='local_interpolation',
                                  NUM_REDUCED_CHANNELS=2, NUM_CHANNELS_OF_LOCAL_AGGREGATION=32, MSG_POST_MLPS=[32],
                                  **GROUPS(0.2, 0.4, 3, [32, 32]))),
    'x_conv3': (20000, 64, dict(NAME='VectorPoolAggregationModuleMSG', NUM_GROUPS=2, LOCAL_AGGREGATION_TYPE='local_interpolation',
                                NUM_REDUCED_CHANNELS=32, NUM_CHANNELS_OF_LOCAL_AGGREGATION=32, MSG_POST_MLPS=[128],
                                **GROUPS(1.2, 2.4, 3, [64, 64]))),
    'x_conv4': (8000, 64, dict(NAME='VectorPoolAggregationModuleMSG', NUM_GROUPS=2, LOCAL_AGGREGATION_TYPE='local_interpolation',
                               NUM_REDUCED_CHANNELS=32, NUM_CHANNELS_OF_LOCAL_AGGREGATION=32, MSG_POST_MLPS=[128],
                               **GROUPS(2.4, 4.8, 3, [64, 64]))),
}
ROI_GRID = dict(NAME='VectorPoolAggregationModuleMSG', NUM_GROUPS=2, LOCAL_AGGREGATION_TYPE='voxel_random_choice',
                NUM_REDUCED_CHANNELS=30, NUM_CHANNELS_OF_LOCAL_AGGREGATION=32, MSG_POST_MLPS=[128],
                GROUP_CFG_0=dict(NUM_LOCAL_VOXEL=[3, 3, 3], MAX_NEIGHBOR_DISTANCE=0.8, NEIGHBOR_NSAMPLE=32, POST_MLPS=[64, 64]),
                GROUP_CFG_1=dict(NUM_LOCAL_VOXEL=[3, 3, 3], MAX_NEIGHBOR_DISTANCE=1.6, NEIGHBOR_NSAMPLE=32, POST_MLPS=[64, 64]))


def timed(fn):
    """median over REPEATS windows of the time of one replay of fn() captured into a graph, in ms"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPLAYS):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / REPLAYS)
    return statistics.median(times), min(times), max(times)


def cloud(rng, B, n, extent):
    xyz = rng.uniform(-1, 1, (B * n, 3)).astype(np.float32) * np.asarray(extent, np.float32)
    return torch.from_numpy(xyz).cuda(), torch.full((B,), n, dtype=torch.int32, device='cuda')


def row(name, ms, tests=None, nbytes=None, **extra):
    out = dict(name=name, ms=round(ms[0], 4), ms_min=round(ms[1], 4), ms_max=round(ms[2], 4), **extra)
    if tests is not None:
        out['point_tests_per_s'] = tests / (ms[0] * 1e-3)
    if nbytes is not None:
        out['bytes'] = int(nbytes)
        out['share_of_hbm_peak'] = nbytes / (ms[0] * 1e-3) / HBM_PEAK
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--small', action='store_true', help='a tenth of the rows and queries (a rehearsal, not a measurement)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_vector_pool.py measures on the GPU: no device found")
    rng = np.random.default_rng(0)
    B, K, scale = 4, 4096 // (10 if args.small else 1), (10 if args.small else 1)
    extent = (30.0, 30.0, 2.0)
    rows = []
    keypoints, key_cnt = cloud(rng, B, K, extent)
    for src, (n, c_in, cfg) in SOURCES.items():
        n //= scale
        sxyz, cnt = cloud(rng, B, n, extent)
        feats = torch.randn(B * n, c_in, device='cuda', requires_grad=True)
        layer, _ = P.build_local_aggregation_module(c_in, cfg)
        layer = layer.cuda().train()
        for k in range(2):
            sub = getattr(layer, f'layer_{k}')
            G, C, dist = sub.total_voxels, sub.num_reduced_channels, sub.max_neighbour_distance
            centers = (keypoints[:, None, :] + sub._grid_offsets[None]).contiguous()
            red = torch.randn(B * n, C, device='cuda')
            M = keypoints.shape[0]
            idx, dist2, ncnt = P.vector_pool_three_nn(sxyz, cnt, keypoints, centers, key_cnt, 2 * dist, -1, 0)
            mean_cnt = float(ncnt.float().mean())
            rows.append(row(f'{src}.group{k}.three_nn', timed(lambda: P.vector_pool_three_nn(sxyz, cnt, keypoints, centers, key_cnt,
                                                                                          2 * dist, -1, 0)),
                            tests=M * n, nbytes=B * n * 12 + M * 12 + M * G * 12 + M * G * 24 + M * 4, G=G, mean_neighbors=mean_cnt))
            out_bytes = M * G * (C + 9) * 4
            rows.append(row(f'{src}.group{k}.interpolate_forward',
                            timed(lambda: P.vector_pool_interpolate(red, idx, dist2, sxyz, centers)),
                            nbytes=M * G * 24 + M * G * 12 + M * G * 3 * (C + 3) * 4 + out_bytes, G=G, C=C))
            g_out = torch.randn(M, G * (C + 9), device='cuda')
            red_g = red.clone().requires_grad_(True)
            y = P.vector_pool_interpolate(red_g, idx, dist2, sxyz, centers)
            rows.append(row(f'{src}.group{k}.interpolate_backward',
                            timed(lambda: torch.autograd.grad(y, red_g, g_out, retain_graph=True)),
                            nbytes=M * G * 24 + M * G * C * 4 + M * G * 3 * C * 8 + B * n * C * 4, G=G, C=C))
        kw = dict(xyz=sxyz, xyz_batch_cnt=cnt, new_xyz=keypoints, new_xyz_batch_cnt=key_cnt, features=feats)

        def step(layer=layer, kw=kw):
            layer.zero_grad(set_to_none=True)
            kw['features'].grad = None
            layer(**kw)[1].square().mean().backward()
        rows.append(row(f'{src}.module_forward_backward', timed(step), rows_per_frame=n, queries=int(keypoints.shape[0])))
    # RoI-grid pooling: 128 x 216 queries per frame over the keypoints
    Mf = 128 * 216 // scale
    centres = keypoints.view(B, K, 3)[:, torch.randint(0, K, (Mf,), device='cuda')]
    new_xyz = (centres + torch.randn(B, Mf, 3, device='cuda') * 0.7).view(-1, 3).contiguous()
    new_cnt = torch.full((B,), Mf, dtype=torch.int32, device='cuda')
    feats = torch.randn(B * K, 90, device='cuda', requires_grad=True)
    layer, _ = P.build_local_aggregation_module(90, ROI_GRID)
    layer = layer.cuda().train()
    for k, dist in enumerate((0.8, 1.6)):
        red = torch.randn(B * K, 30, device='cuda', requires_grad=True)
        args_ = (keypoints, key_cnt, red, new_xyz, new_cnt, 3, 3, 3, dist, 30, 1, 20, 32, 0, 1)
        out, _, _, pc = P.vector_pool_with_voxel_query_op(*args_)
        M = new_xyz.shape[0]
        nbytes = B * K * 12 + M * 12 + M * 27 * (30 + 3 + 2) * 4 + float(pc.sum()) * 30 * 4
        rows.append(row(f'roi_grid.group{k}.voxel_query_forward', timed(lambda: P.vector_pool_with_voxel_query_op(*args_)),
                        tests=M * K, nbytes=nbytes, filled_cells_per_query=float(pc.sum()) / M))
        g_out = torch.randn_like(out)
        rows.append(row(f'roi_grid.group{k}.voxel_query_backward',
                        timed(lambda: torch.autograd.grad(out, red, g_out, retain_graph=True)),
                        nbytes=M * 27 * (30 + 1) * 4 + float(pc.sum()) * 30 * 8))
    kw = dict(xyz=keypoints, xyz_batch_cnt=key_cnt, new_xyz=new_xyz, new_xyz_batch_cnt=new_cnt, features=feats)

    def step():
        layer.zero_grad(set_to_none=True)
        feats.grad = None
        layer(**kw)[1].square().mean().backward()
    rows.append(row('roi_grid.module_forward_backward', timed(step), rows_per_frame=K, queries=int(new_xyz.shape[0])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), batch=B, keypoints_per_frame=K, repeats=REPEATS,
                           replays_per_window=REPLAYS, small=bool(args.small), rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
