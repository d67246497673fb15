"""Does a SubM layer run on the window tiles (spconv_win.hip)?  The one place that knows the bits of the "subm_window" and
"subm_window_wgrad" options; the layers, the rulebook builds, the backbones' prefetcher and the backward pass all ask here."""
import torch

from .. import _lib as L
from .. import ops

# "subm_window": the widths whose forward / data gradient may run on the window tiles; _PADDED: so may a layer with fewer input
# than output channels, on rows zero-padded to the kernel's width (forward and weight gradient only)
_FWD_BITS = {64: 1, 32: 2, 16: 4, 128: 8}
_PADDED = 16
_WGRAD_BITS = {64: 1, 32: 2, 16: 4}               # "subm_window_wgrad": the widths whose weight gradient may


def capable(conv):
    """A window kernel exists for this layer and the "subm_window" option admits it."""
    cin, cout = conv.in_channels, conv.out_channels
    if not (conv.subm and tuple(conv.kernel_size) == (3, 3, 3) and tuple(conv.dilation) == (1, 1, 1) and cin <= cout):
        return False
    opt = L.get_option("subm_window")
    return (bool(opt & _FWD_BITS.get(cout, 0)) and (cin == cout or bool(opt & _PADDED))
            and ops.subm_window_tile_rows(cout, cout) > 0)


def window_wgrad(c):
    """The "subm_window_wgrad" option admits the window weight gradient for c channels."""
    return bool(L.get_option("subm_window_wgrad") & _WGRAD_BITS.get(int(c), 0))


def forward_on_tiles(conv, order, dtype=None, cols=None, dgrad_due=False):
    """Forward and data gradient of `conv` run on the window tiles: a capable layer, a rulebook over z-fastest rows (`order`),
    bf16 features `cols` wide -- the layer's width or, with fewer input channels (conv_input: 5 -> 16), rows zero-padded to a
    kernel width, and then no data gradient due.  dtype / cols None: not known yet (a rulebook is built ahead of the features
    of the layers that share it), taken to fit.  A layer's fp8 training form is the caller's to rule out."""
    padded = conv.in_channels < conv.out_channels
    return (order == ops.ROWS_YXZ and dtype in (None, torch.bfloat16)
            and (cols is None or cols == conv.in_channels or
                 (padded and cols in (ops.pow2_ge8(conv.in_channels), conv.out_channels)))
            and not (padded and dgrad_due) and capable(conv))


def wgrad_on_tiles(fwd, cin, cout, cols=None):
    """The weight gradient runs over the window tiles too: behind a window forward (`fwd`) whose saved rows (`cols` wide; None:
    as that forward pads them) are as wide as its output."""
    return bool(fwd) and cin <= cout and cols in (None, cout) and window_wgrad(cout)
