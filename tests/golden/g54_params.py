"""Deterministic parameters of the G54 end-to-end fixture for UNetV2 (shared by make_golden_unet.py, which runs the dense
conv3d / conv_transpose3d / BatchNorm1d chain with them, and by the tests, which load them into the HIP module).  The G7
method (g7_params.py) applied to pcdet/models/backbones_3d/spconv_unet.py:49-212.

Geometry: grid (x, y, z) = (48, 64, 24) -> sparse shape (25, 64, 48): non-square, and the smallest grid that survives the
chain, (25,64,48) -> (13,32,24) -> (7,16,12) -> (3,8,6) -> conv_out (1,8,6); conv4 has padding (0, 1, 1)."""
import zlib

import numpy as np

SEED = 20250954
RANGE = (-2.4, -3.2, -1.6, 2.4, 3.2, 2.0)
VOXEL = (0.1, 0.1, 0.15)
GRID = (48, 64, 24)
BATCH = 2
POINTS_PER_FRAME = 3600
MAX_POINTS, MAX_VOXELS = 5, 4000
IN_CHANNELS = 5
BN_EPS, BN_MOMENTUM = 1e-3, 0.01                # spconv_unet.py:63
LOSS_QUAD = 64.0                                # loss = LOSS_QUAD * 0.5 * (mean(sf^2) + mean(pf^2)) + <sf, P> + <pf, Q>

# encoder (spconv_unet.py:65-106): VoxelBackBone8x layer for layer
ENCODER = (
    dict(kind="subm", name="conv_input", cin=IN_CHANNELS, cout=16),
    dict(kind="subm", name="conv1.0", cin=16, cout=16, tap="x_conv1"),
    dict(kind="spconv", name="conv2.0", cin=16, cout=32, k=(3, 3, 3), s=(2, 2, 2), p=(1, 1, 1)),
    dict(kind="subm", name="conv2.1", cin=32, cout=32),
    dict(kind="subm", name="conv2.2", cin=32, cout=32, tap="x_conv2"),
    dict(kind="spconv", name="conv3.0", cin=32, cout=64, k=(3, 3, 3), s=(2, 2, 2), p=(1, 1, 1)),
    dict(kind="subm", name="conv3.1", cin=64, cout=64),
    dict(kind="subm", name="conv3.2", cin=64, cout=64, tap="x_conv3"),
    dict(kind="spconv", name="conv4.0", cin=64, cout=64, k=(3, 3, 3), s=(2, 2, 2), p=(0, 1, 1)),
    dict(kind="subm", name="conv4.1", cin=64, cout=64),
    dict(kind="subm", name="conv4.2", cin=64, cout=64, tap="x_conv4"),
)
CONV_OUT = dict(kind="spconv", name="conv_out", cin=64, cout=128, k=(3, 1, 1), s=(2, 1, 1), p=(0, 0, 0))
# decoder (spconv_unet.py:110-132, 198-204): (level, channels C of the lateral, output channels of the last block, its module,
# the strided layer whose rulebook the inverse conv shares -- None: conv5, a SubM block)
DECODER = (
    dict(level=4, c=64, cout=64, last="inv_conv4", strided="conv4.0", tap="x_up4"),
    dict(level=3, c=64, cout=32, last="inv_conv3", strided="conv3.0", tap="x_up3"),
    dict(level=2, c=32, cout=16, last="inv_conv2", strided="conv2.0", tap="x_up2"),
    dict(level=1, c=16, cout=16, last="conv5.0", strided=None, tap="x_up1"),
)
TAP_NAMES = ("x_conv1", "x_conv2", "x_conv3", "x_conv4", "out", "x_up4", "x_up3", "x_up2", "x_up1")


def param_specs():
    """[(state-dict name, shape, kind)] in the module order of spconv_unet.py."""
    out = []

    def conv(name, cout, k, cin):
        out.append((name + ".weight", (cout,) + tuple(k) + (cin,), "w"))

    def bn(prefix, c):
        out.append((prefix + ".weight", (c,), "gamma"))
        out.append((prefix + ".bias", (c,), "beta"))

    for L in ENCODER + (CONV_OUT,):
        conv(L["name"] + ".0", L["cout"], L.get("k", (3, 3, 3)), L["cin"])
        bn(L["name"] + ".1", L["cout"])
    for D in DECODER:
        lv, c = D["level"], D["c"]
        for j in (1, 2):
            conv(f"conv_up_t{lv}.conv{j}", c, (3, 3, 3), c)
            bn(f"conv_up_t{lv}.bn{j}", c)
        conv(f"conv_up_m{lv}.0", c, (3, 3, 3), 2 * c)
        bn(f"conv_up_m{lv}.1", c)
        conv(D["last"] + ".0", D["cout"], (3, 3, 3), c)
        bn(D["last"] + ".1", D["cout"])
    return out


def make_param(name, shape, kind):
    rng = np.random.default_rng([SEED, zlib.crc32(name.encode())])
    if kind == "w":
        fan_in = int(np.prod(shape[1:]))
        bound = np.sqrt(6.0 / ((1 + 5.0) * fan_in))          # kaiming_uniform_(a=sqrt(5))
        return rng.uniform(-bound, bound, shape).astype(np.float32)
    if kind == "gamma":
        return rng.uniform(0.5, 1.5, shape).astype(np.float32)
    if kind == "beta":
        return rng.uniform(-0.3, 0.3, shape).astype(np.float32)
    raise ValueError(kind)


def state_dict():
    return {name: make_param(name, shape, kind) for name, shape, kind in param_specs()}


def _bf16_values(p):
    u = p.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def loss_projection(numel, which=99):
    """Fixed projection (bf16-representable values); which = 99: over the BEV map, 98: over point_features."""
    rng = np.random.default_rng([SEED, which])
    return _bf16_values((rng.normal(size=numel) * 1e-2).astype(np.float32))


def sample(a, cap):
    """What the fixture keeps of a tensor: everything up to `cap` elements, else a strided subsample (odd stride: every
    channel of a [rows, channels] matrix with an even channel count is visited)."""
    flat = np.asarray(a).reshape(-1)
    stride = max(1, -(-flat.size // cap)) | 1 if flat.size > cap else 1
    return flat[::stride]


def grad_sample(g):
    return sample(g, 2048)


def tap_sample(t):
    return sample(t, 4096)


def points(seed, n, batch):
    """Clustered cloud on the reduced grid, g7_params.points style (some points out of range / exactly on faces), coordinates
    on a 2^-10 lattice so the stored frames compress."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(batch):
        ctr = rng.uniform(-1.0, 1.0, (10, 3)) * np.array([1.9, 2.6, 0.5])
        which = rng.integers(0, 10, n)
        p = ctr[which] + rng.normal(0, 0.3, (n, 3)) * np.array([1, 1, 0.6])
        p[: n // 20] = rng.uniform(-3.5, 3.5, (n // 20, 3))
        p[n // 20] = [-2.4, 0.0, 0.0]
        p[n // 20 + 1] = [2.4, 0.0, 0.0]
        p[n // 20 + 2] = [0.0, 0.0, 2.0]
        p[n // 20 + 3] = [0.3, -0.7, -1.6]
        feat = np.concatenate([p, np.tanh(rng.uniform(0, 2, (n, 1))), rng.uniform(0, 1.5, (n, 1))], 1)
        out.append((np.round(feat * 1024) / 1024).astype(np.float32))
    return out
