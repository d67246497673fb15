"""The four dense convs of the BEV stack -- ops.DENSE_KINDS: nn.Conv2d(3, stride 1, padding 1), nn.Conv2d(3, stride 2,
padding 1) and nn.ConvTranspose2d(k = stride in {1, 2}) -- on channels-last bf16 maps through the hand-written kernels of
com_amd/csrc/conv2d.hip instead of MIOpen: forward and data gradient are the same MFMA kernel family (weights packed with the
kind's forward mode / the next odd one), the weight gradient is the dense 3x3 kernel or the sparse path's pair-wise X^T dY
kernel (spconv.hip) run over the DENSE pair lists of the kind's taps -- built once per map shape.  `Conv3x3`, `Conv3x3S2` and
`UpConvT` are drop-in subclasses (same parameters and state-dict keys, base_bev_backbone.py:37-62 / center_head.py:17-24
construct them with the same arguments); anything the kernels do not cover (`_covered`: other kernel sizes / strides,
cin % 32 != 0, ...; `_fast`: CPU tensors, fp32 maps outside a bf16 autocast region) takes torch's own path."""
import torch
import torch.nn as nn

from .. import ops
from ..spconv import functional as Fsp

ENABLED = True
# The following BatchNorm's statistics are taken in the dense conv's epilogue (PcdBnReduce mode 1 of pcd_conv2d_3x3_nhwc_bn)
# whenever spconv.functional.FUSE_BN_REDUCTIONS holds.  Measured in the full step (2 x 80 replays): off 7.84, forward
# 7.79 ms.  The backward reductions on the data-gradient launch (mode 2) were retired: they re-read the BatchNorm's input
# and output tile in that epilogue and lost, 7.89 ms alone and 7.86 with the forward form.
BATCH_BN_COUNTERS = True
_PAIRS = {}


def pair_lists(mode, B, H, W, device):
    """indice_pairs for the WEIGHT gradient of the dense kind `mode` on a [B, H, W] input map, in the (gathered row,
    accumulated row) convention of the sparse pair kernels, built once per map shape: the pairs of the ordinary convolution
    (k, s, p) from the kind's fine map [fh, fw] to its coarse one -- tap t = ty * k + tx pairs the fine pixel
    (s oy + ty - p, s ox + tx - p) with the coarse pixel (oy, ox); row = (b * height + y) * width + x.  For a conv the fine
    map is x and dW comes out as [cout, K, cin]; for a transposed conv it is dy, the kernel runs with the roles of x / dy
    swapped and dW comes out as [cin, K, cout], the parameter's own layout.  Returns pairs [K, 2, n] (valid ones first,
    ascending; -1 behind) and pair_num [K]."""
    key = (mode, B, H, W, str(device))
    hit = _PAIRS.get(key)
    if hit is not None:
        return hit
    kind = ops.DENSE_KINDS[mode]
    k, s, p = kind.k, kind.stride, kind.pad
    fh, fw = kind.fine_hw(H, W)
    ch, cw = (fh + 2 * p - k) // s + 1, (fw + 2 * p - k) // s + 1
    n = B * ch * cw
    o = torch.arange(n, device=device, dtype=torch.int64)
    b, oy, ox = o // (ch * cw), (o // cw) % ch, o % cw
    pairs = torch.full((k * k, 2, n), -1, dtype=torch.int32, device=device)
    num = torch.zeros((k * k,), dtype=torch.int32, device=device)
    for t in range(k * k):
        fy, fx = s * oy + t // k - p, s * ox + t % k - p
        ok = (fy >= 0) & (fy < fh) & (fx >= 0) & (fx < fw)
        m = int(ok.sum())
        pairs[t, 0, :m] = ((b * fh + fy) * fw + fx)[ok].int()
        pairs[t, 1, :m] = o[ok].int()
        num[t] = m
    _PAIRS[key] = (pairs, num)
    return pairs, num


def _dense_pairs(B, H, W, device):
    """The pair lists of the 3x3 / stride 1 / padding 1 conv (kind 0)."""
    return pair_lists(0, B, H, W, device)


def _pad32(c):
    return (c + 31) // 32 * 32


def _bf16_region(x):
    return x.is_cuda and (x.dtype == torch.bfloat16 or (torch.is_autocast_enabled()
                                                        and torch.get_autocast_dtype('cuda') == torch.bfloat16))


def dense_input(x):
    """x as the kernels read it -- bf16, channels-last storage -- or None for a map they do not take: off the device, or
    fp32 outside a bf16 autocast region."""
    if not _bf16_region(x):
        return None
    if x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)
    if not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    return x


def _grad_nhwc(dy, cp):
    """dy [B, cout, H, W] as the backward kernels read it: [B, H, W, cp] bf16 contiguous, zero-padded to cp channels."""
    dyn = dy.permute(0, 2, 3, 1)
    if dyn.dtype != torch.bfloat16:
        dyn = dyn.to(torch.bfloat16)
    if cp != dyn.shape[3]:
        dyn = torch.nn.functional.pad(dyn, (0, cp - dyn.shape[3]))
    return dyn.contiguous()


def _wgrad_3x3(x, dyp, weight, wp, direct, jobs, x_block=False):
    """dW of ONE 3x3 / stride 1 conv: x [B, H, W, cin] bf16 (x_block: a channel block of a wider map), dyp [B, H, W, cp] its
    output gradient with zero-padded channels.  direct: into wp.grad (slab reduction deferred to `jobs`; only the real rows
    of the slabs are reduced), returns None; otherwise returns a tensor in the parameter's layout and dtype."""
    B, H, W, cin = x.shape
    cout, cp = weight.shape[0], dyp.shape[3]
    if ops.conv2d_wgrad_splits(B, H, W, cin, cp) > 0:              # the dense kernel (no pair lists)
        if direct:
            ops.conv2d_wgrad(x, dyp, cout, out=wp.grad, defer=jobs)
            return None
        return ops.conv2d_wgrad(x, dyp, cout).to(weight.dtype)
    pairs, num = _dense_pairs(B, H, W, x.device)
    rows = x.view(-1, cin)                                          # (a channel block stays one: row stride of the wide map)
    if direct:
        ops.wgrad(rows, cin, dyp.reshape(-1, cp), pairs, num, 9, out=wp.grad, defer=jobs, conv2d_layout=True,
                  cout_write=cout if cp != cout else 0, x_block=x_block)
        return None
    dwk = ops.wgrad(rows, cin, dyp.reshape(-1, cp), pairs, num, 9, x_block=x_block)      # [cp, 9, cin] f32
    return dwk[:cout].permute(0, 2, 1).reshape(cout, cin, 3, 3).to(weight.dtype)


def _bias_grad(dyp, cout, bp, direct):
    """Column sums of dyp [B, H, W, cp] (fp32, fixed order), the first cout of them: into bp.grad (direct) or returned."""
    cp = dyp.shape[3]
    if direct and cp == cout:
        ops.col_sum(dyp.reshape(-1, cp), out=bp.grad)
        return None
    cs = ops.col_sum(dyp.reshape(-1, cp))[:cout]
    if direct:
        bp.grad.copy_(cs)
        return None
    return cs


class _DenseConv:
    """What Conv3x3, Conv3x3S2 and UpConvT share: the covering predicate and the packs made ahead."""
    KINDS = ()           # forward pack modes of the kinds the class can stand for

    def _covered(self):
        """The forward pack mode of the dense kind whose kernels cover this module, or None -- by the module alone: what
        `_fast` asks of it and what Conv3x3Packs plans by."""
        for mode in self.KINDS:
            kind = ops.DENSE_KINDS[mode]
            if (self.kernel_size == (kind.k, kind.k) and self.stride == (kind.stride, kind.stride)
                    and self.padding == (kind.pad, kind.pad) and self.output_padding == (0, 0) and self.dilation == (1, 1)
                    and self.groups == 1 and self.padding_mode == 'zeros' and (kind.bias or self.bias is None)
                    and self.in_channels % 32 == 0 and (kind.any_cout or self.out_channels % 32 == 0)):
                return mode
        return None

    def _fast(self, x):
        return (ENABLED and _bf16_region(x) and x.dim() == 4 and (mode := self._covered()) is not None
                and x.shape[0] * x.shape[2] * x.shape[3] * ops.DENSE_KINDS[mode].span
                * max(self.in_channels, _pad32(self.out_channels)) * 2 < 2 ** 32 - 4096)

    def _take_packs(self):
        """(pack_f, pack_d) made ahead by Conv3x3Packs.run() since the last weight update, or (None, None)."""
        pf = pd = None
        ahead = getattr(self, "_packs_ahead", None)
        if ahead is not None:                        # use them ONCE
            self._packs_ahead = None
            if ahead[2] == self.weight._version:     # (an in-place change since run() -- load_state_dict, broadcast,
                pf, pd = ahead[0], ahead[1]          #  a manual edit -- bumps the version: pack again from the weights)
        return pf, pd


class _Conv3x3Function(torch.autograd.Function):
    """Output channel counts that are not a multiple of 32 (the 1 / 2 / 3-channel final convs of the head towers) run
    padded with zero weights (the packs carry the padding): MIOpen spends 0.4 ms on each of those tiny convs.
    pack_f / pack_d: packs made ahead (Conv3x3Packs), or None: packed here."""

    @staticmethod
    def forward(ctx, x, weight, bias, pack_f, pack_d, bn_follows=False):
        # x: [B, C, H, W] bf16, channels_last storage
        # bn_follows: a training-mode BatchNorm consumes the output -> its statistics are taken in this launch's epilogue
        xn = x.detach().permute(0, 2, 3, 1)
        assert xn.is_contiguous()
        cout = weight.shape[0]
        cp = _pad32(cout)
        b = bias.detach().float() if bias is not None else None
        if b is not None and cp != cout:
            b = torch.nn.functional.pad(b, (0, cp - cout))
        if pack_f is None:
            pack_f = ops.conv2d_pack_weight(weight, 0)
        stats = ops.BnReduce(1) if (bn_follows and Fsp.FUSE_BN_REDUCTIONS and cp == cout) else None
        y = ops.conv2d_3x3_nhwc(xn, pack_f, cp, b, bn_reduce=stats)
        if cp != cout:
            y = y[..., :cout].contiguous()
        ctx.save_for_backward(xn, weight, pack_d)
        ctx.has_bias, ctx.cout = bias is not None, cout
        ctx.weight_param = weight if isinstance(weight, nn.Parameter) else None
        ctx.bias_param = bias if isinstance(bias, nn.Parameter) else None
        out = y.permute(0, 3, 1, 2)
        if stats is not None and stats.partial is not None:
            out._pcd_stats = stats
        return out

    @staticmethod
    def backward(ctx, dy):
        xn, weight, pack_d = ctx.saved_tensors
        cin, cout = xn.shape[3], ctx.cout
        dyn = _grad_nhwc(dy, _pad32(cout))
        wp, bp = ctx.weight_param, ctx.bias_param

        def dgrad():
            pd = pack_d if pack_d is not None else ops.conv2d_pack_weight(weight, 1)
            return ops.conv2d_3x3_nhwc(dyn, pd, cin).permute(0, 3, 1, 2)

        dx, dw, db = Fsp.scheduled_backward(
            ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2], wp, bp, dgrad,
            lambda direct, jobs: _wgrad_3x3(xn, dyn, weight, wp, direct, jobs),
            lambda direct, jobs: _bias_grad(dyn, cout, bp, direct), [xn, dyn])
        return dx, dw, db, None, None, None


class _ConvPlanesFunction(torch.autograd.Function):
    """The stride-2 3x3 conv (mode 2) and the k = stride transposed convs (modes 4, 6) of BaseBEVBackbone through the
    plane kernels of conv2d.hip; the data gradient is the same kernel family with the next odd pack mode, the weight
    gradient the sparse pair kernels over dense pair lists (pair_lists).  No bias (base_bev_backbone.py:38,58,66)."""

    @staticmethod
    def forward(ctx, x, weight, pack_f, pack_d, mode_f):
        xn = x.detach().permute(0, 2, 3, 1)
        assert xn.is_contiguous()
        kind = ops.DENSE_KINDS[mode_f]
        if pack_f is None:
            pack_f = ops.conv2d_pack_weight(weight, mode_f)
        y = ops.conv2d_planes_nhwc(mode_f, xn, pack_f, kind.channels(weight)[1], kind.out_hw(xn.shape[1], xn.shape[2]))
        ctx.save_for_backward(xn, weight, pack_d)
        ctx.mode_f = mode_f
        ctx.weight_param = weight if isinstance(weight, nn.Parameter) else None
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        xn, weight, pack_d = ctx.saved_tensors
        mode_f = ctx.mode_f
        kind = ops.DENSE_KINDS[mode_f]
        B, H, W, cin = xn.shape
        cout = kind.channels(weight)[1]
        dyn = _grad_nhwc(dy, cout)
        wp = ctx.weight_param

        def dgrad():
            pd = pack_d if pack_d is not None else ops.conv2d_pack_weight(weight, mode_f + 1)
            return ops.conv2d_planes_nhwc(mode_f + 1, dyn, pd, cin, (H, W)).permute(0, 3, 1, 2)

        def wgrad(direct, jobs):
            pairs, num = pair_lists(mode_f, B, H, W, xn.device)
            # gathered rows (contraction c) = the fine map, accumulated rows (o) = the coarse one: x and dy for a conv, swapped
            # for a transposed conv -> dW [o, K, c] = the parameter's layout either way
            a, ca, b_, cb = xn.reshape(-1, cin), cin, dyn.reshape(-1, cout), cout
            if kind.transposed:
                a, ca, b_, cb = b_, cb, a, ca
            if direct:
                ops.wgrad(a, ca, b_, pairs, num, kind.taps, out=wp.grad, defer=jobs, conv2d_layout=True)
                return None
            dwk = ops.wgrad(a, ca, b_, pairs, num, kind.taps)             # [cb, K, ca] f32
            return dwk.permute(0, 2, 1).reshape(cb, ca, kind.k, kind.k).to(weight.dtype)

        dx, dw, _ = Fsp.scheduled_backward(ctx.needs_input_grad[0], ctx.needs_input_grad[1], False, wp, None, dgrad,
                                           wgrad, None, [xn, dyn])
        return dx, dw, None, None, None


class Conv3x3(_DenseConv, nn.Conv2d):
    """nn.Conv2d whose forward takes the HIP kernel when it applies (see the module docstring)."""
    KINDS = (0,)
    bn_follows = False   # set by the owner when a BatchNormReLU2d consumes the output (dense2d.py)

    def forward(self, x):
        if not self._fast(x):
            return super().forward(x)
        pf, pd = self._take_packs()
        follows = bool(self.bn_follows and self.training and torch.is_grad_enabled())
        return _Conv3x3Function.apply(dense_input(x), self.weight, self.bias, pf, pd, follows)


class Conv3x3S2(_DenseConv, nn.Conv2d):
    """nn.Conv2d(k = 3, stride 2, padding 1, bias=False) -- the conv that opens a down-sampling block
    (base_bev_backbone.py:36-41: ZeroPad2d(1) + Conv2d(padding=0), the same arithmetic) -- through the plane kernels."""
    KINDS = (2,)

    def forward(self, x):
        if not self._fast(x):
            return super().forward(x)
        pf, pd = self._take_packs()
        return _ConvPlanesFunction.apply(dense_input(x), self.weight, pf, pd, self.KINDS[0])


class UpConvT(_DenseConv, nn.ConvTranspose2d):
    """nn.ConvTranspose2d(k = stride in {1, 2}, bias=False) -- the deblocks (base_bev_backbone.py:55-62) -- through the
    plane kernels (k = 2: four 1-tap planes written with stride 2, no intermediate + pixel shuffle pass)."""
    KINDS = (4, 6)

    def forward(self, x, output_size=None):
        if output_size is not None or not self._fast(x):
            return super().forward(x, output_size)
        pf, pd = self._take_packs()
        return _ConvPlanesFunction.apply(dense_input(x), self.weight, pf, pd, self._covered())


class _BranchConvsFunction(torch.autograd.Function):
    """The LAST 3x3 convs (64 -> 1..3 channels, bias) of all branches of a SeparateHead (center_head.py:21-24) on the
    channel blocks of ONE shared activation a [B, 64 n, H, W]: branch i reads channels [64 i, 64 i + 64) in place, its data
    gradient fills that block of da -- no slice copies forward, no zero-filled slice gradients and no adds backward.
    Outputs are the first cout_i channels of maps computed with zero-padded output channels (views, pixel stride 32).
    metas[i] = (pack_f, pack_d) made ahead or (None, None); wb = w_0, b_0, w_1, b_1, ..."""

    @staticmethod
    def forward(ctx, a, width, metas, *wb):
        an = a.detach().permute(0, 2, 3, 1)
        assert an.is_contiguous() and an.shape[3] == width * (len(wb) // 2)
        outs, packs_d = [], []
        for i in range(len(wb) // 2):
            w, b = wb[2 * i], wb[2 * i + 1]
            cout = w.shape[0]
            cp = _pad32(cout)
            bp = torch.nn.functional.pad(b.detach().float(), (0, cp - cout)) if b is not None else None
            pf = metas[i][0] if metas[i][0] is not None else ops.conv2d_pack_weight(w, 0)
            y = ops.conv2d_3x3_nhwc(an[..., width * i:width * (i + 1)], pf, cp, bp)
            outs.append(y[..., :cout].permute(0, 3, 1, 2))
            packs_d.append(metas[i][1])
        ctx.save_for_backward(an, *[wb[2 * i] for i in range(len(wb) // 2)])
        ctx.width, ctx.packs_d = width, packs_d
        ctx.w_params = [wb[2 * i] if isinstance(wb[2 * i], nn.Parameter) else None for i in range(len(wb) // 2)]
        ctx.b_params = [wb[2 * i + 1] if isinstance(wb[2 * i + 1], nn.Parameter) else None for i in range(len(wb) // 2)]
        ctx.has_bias = [wb[2 * i + 1] is not None for i in range(len(wb) // 2)]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dys):
        an, ws = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        B, H, W, C = an.shape
        n, width = len(ws), ctx.width
        cps = [_pad32(w.shape[0]) for w in ws]
        # the output gradients, zero-padded to the channel count the kernels contract over: ONE fill + n copies
        pad = torch.zeros((sum(cps) * B * H * W,), dtype=torch.bfloat16, device=an.device)
        dyp, off = [], 0
        for i in range(n):
            t = pad[off:off + cps[i] * B * H * W].view(B, H, W, cps[i])
            off += cps[i] * B * H * W
            if dys[i] is not None:
                t[..., :ws[i].shape[0]].copy_(dys[i].permute(0, 2, 3, 1))
            dyp.append(t)
        live = [i for i in range(n) if dys[i] is not None]
        want_w = any(ctx.needs_input_grad[3 + 2 * i] for i in live)
        want_b = any(ctx.has_bias[i] and ctx.needs_input_grad[4 + 2 * i] for i in live)

        def dgrad():
            da = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=an.device)
            for i in range(n):
                blk = da[..., width * i:width * (i + 1)]
                if dys[i] is None:
                    blk.zero_()
                    continue
                pd = ctx.packs_d[i] if ctx.packs_d[i] is not None else ops.conv2d_pack_weight(ws[i], 1)
                ops.conv2d_3x3_nhwc(dyp[i], pd, width, out=blk)
            return da.permute(0, 3, 1, 2)

        def wgrad(direct, jobs):
            return [_wgrad_3x3(an[..., width * i:width * (i + 1)], dyp[i], ws[i], ctx.w_params[i], direct, jobs, x_block=True)
                    if dys[i] is not None and ctx.needs_input_grad[3 + 2 * i] else None for i in range(n)]

        def bsum(direct, jobs):
            return [_bias_grad(dyp[i], ws[i].shape[0], ctx.b_params[i], direct)
                    if dys[i] is not None and ctx.has_bias[i] and ctx.needs_input_grad[4 + 2 * i] else None for i in range(n)]

        wps = [ctx.w_params[i] for i in live if ctx.needs_input_grad[3 + 2 * i]]
        bps = [ctx.b_params[i] for i in live if ctx.has_bias[i] and ctx.needs_input_grad[4 + 2 * i]]
        dx, dws, dbs = Fsp.scheduled_backward(ctx.needs_input_grad[0], want_w, want_b, wps, bps, dgrad, wgrad, bsum,
                                              [an, pad])
        grads = [dx, None, None]
        for i in range(n):
            grads.append(dws[i] if dws is not None else None)
            grads.append(dbs[i] if dbs is not None else None)
        return tuple(grads)


class Conv3x3Packs:
    """Forward + data-gradient packs of all Conv3x3 / Conv3x3S2 / UpConvT modules of a model that the kernels cover
    (`_covered`) in ONE launch (pcd_conv2d_pack_weights_batched) into persistent buffers -- call `run()` right after every
    optimizer step (the weights do not change again before the next forward; 2 x 22 small pack launches otherwise sit in
    front of the convs of the CenterPoint BEV stack).
    A module uses the packs for exactly one forward / backward and packs by itself again afterwards, so a forgotten
    `run()` costs time, never correctness; packs made BEFORE a torch-visible in-place change of the weight
    (load_state_dict, checkpoint restore, dist.broadcast, manual edits: all bump `weight._version`) are dropped."""

    def __init__(self, model):
        from .. import _lib as L
        self.convs, self.modes = [], []
        extra = []
        for m in model.modules():
            hook = getattr(m, "_pack_extra_convs", None)       # (SeparateHead: its batched first-stage conv, if any)
            if callable(hook):
                extra += list(hook())
        for m in list(model.modules()) + extra:
            mode = m._covered() if isinstance(m, _DenseConv) else None
            if mode is not None and m.weight.is_cuda and m.weight.dtype == torch.float32:
                self.convs.append(m), self.modes.append((mode, mode + 1))
        rows, first, self.bufs = [], 0, []
        lib = L.lib()
        for m, modes in zip(self.convs, self.modes):
            cin, cout = m.in_channels, m.out_channels
            pair = []
            for mode in modes:
                nbytes = lib.pcd_conv2d_packed_weight_bytes(cin, cout, mode)
                buf = torch.empty((nbytes // 2,), dtype=torch.bfloat16, device=m.weight.device)
                rows.append([m.weight.data_ptr(), buf.data_ptr(), cin, cout, _pad32(cout), mode, first, nbytes // 16])
                first += (nbytes // 16 + 255) // 256
                pair.append(buf)
            self.bufs.append(tuple(pair))
        self.total_blocks = first
        self.keys = tuple(m.weight.data_ptr() for m in self.convs)
        self.table = torch.tensor(rows, dtype=torch.int64).to(self.convs[0].weight.device) if rows else None

    def run(self):
        from .. import _lib as L
        if self.table is None:
            return
        if self.keys != tuple(m.weight.data_ptr() for m in self.convs):
            raise L.PcdError("Conv3x3Packs: a weight moved since the plan was built (build a new plan)")
        L.check(L.lib().pcd_conv2d_pack_weights_batched(L.ptr(self.table), len(self.convs) * 2, self.total_blocks,
                                                        L.stream_ptr()), "pcd_conv2d_pack_weights_batched")
        for m, pair in zip(self.convs, self.bufs):
            m._packs_ahead = (pair[0], pair[1], m.weight._version)


class BatchNormReLU2d(nn.BatchNorm2d):
    """nn.BatchNorm2d (+ the nn.ReLU behind it when relu=True) on channels-last bf16 maps through the fused BatchNorm
    kernels of the sparse path (fused.hip: a [B, H, W, C] map is the same [rows, C] matrix as a sparse tensor's
    features) -- two streaming passes forward, two backward, ReLU included, instead of MIOpen's BatchNorm kernels plus
    an elementwise ReLU each way.  Same parameters / buffers / state-dict keys as nn.BatchNorm2d
    (base_bev_backbone.py:40-41,49-50, center_head.py:19-20); other inputs take nn.BatchNorm2d's own path."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, relu=False):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=affine,
                         track_running_stats=track_running_stats)
        self.relu = bool(relu)

    def forward(self, x, out=None):
        """out (optional): a [B, C, H, W] channel block of a wider channels-last map; when the fused training path
        runs, y is written THERE (self.wrote_out = True) and the returned tensor is that view -- otherwise `out` is
        ignored and the caller concatenates as usual."""
        self.wrote_out = False
        if ENABLED and x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16 \
                and x.is_contiguous(memory_format=torch.channels_last):
            B, C, H, W = x.shape
            rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
            if Fsp._fusable(self, rows):
                out_rows = None
                if out is not None and self.training and self.relu and self.bias is not None \
                        and out.shape == x.shape and out.dtype == x.dtype and out.stride(1) == 1:
                    out_rows = out.permute(0, 2, 3, 1).reshape(B * H * W, C)
                    if out_rows.data_ptr() != out.data_ptr() or out_rows.stride(1) != 1:
                        out_rows = None                                   # (reshape had to copy: not a column block)
                st = getattr(x, "_pcd_stats", None)           # the conv in front took the statistics in its epilogue
                if st is not None:
                    rows._pcd_stats = st
                y = Fsp.batch_norm_act(self, rows, None, self.relu, out=out_rows)
                self.wrote_out = out_rows is not None
                return y.view(B, H, W, C).permute(0, 3, 1, 2)
        if getattr(self, "_defer_nbt", False) and self.training and self.num_batches_tracked is not None:
            self.num_batches_tracked.sub_(1)         # bump_bn_counters() already counted this call
        y = super().forward(x)
        return torch.relu(y) if self.relu else y


class ConcatChannelBlocks(torch.autograd.Function):
    """torch.cat(parts, dim=1) when the parts already ARE the channel blocks of `wide` (each BatchNorm wrote its output
    there): returns `wide`, no copy; backward hands every part its channel block of the gradient as a view."""

    @staticmethod
    def forward(ctx, wide, *parts):
        off = 0
        for p in parts:
            assert p.data_ptr() == wide.data_ptr() + off * wide.element_size() and p.stride() == wide.stride()
            off += p.shape[1]
        assert off == wide.shape[1]
        ctx.widths = [p.shape[1] for p in parts]
        return wide.view_as(wide)

    @staticmethod
    def backward(ctx, g):
        outs, off = [None], 0
        for w in ctx.widths:
            outs.append(g[:, off:off + w])
            off += w
        return tuple(outs)


def bump_bn_counters(module):
    """num_batches_tracked += 1 for every BatchNormReLU2d below `module` in ONE multi-tensor launch (the modules then
    skip their own increment): 20 one-element launches per step otherwise sit between the convs of the BEV stack."""
    if not BATCH_BN_COUNTERS:
        return
    bns = module.__dict__.get("_bn2d_list")
    if bns is None:
        bns = [m for m in module.modules() if isinstance(m, BatchNormReLU2d)]
        for m in bns:
            m._defer_nbt = True
        module.__dict__["_bn2d_list"] = bns
    if module.training:
        counters = [m.num_batches_tracked for m in bns if m.num_batches_tracked is not None]
        if counters:
            torch._foreach_add_(counters, 1)
