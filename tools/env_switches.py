"""Experiment switches of bench.py and the tools: environment variables -> module attributes / library options.

The product modules (com_amd/**) and the library read NO environment variable; their tunables are plain attributes with the
measured optimum as default and `pcd_set_option`.  The scripts that sweep them (tools/*.sh, bench.py children) pass values
through the environment -- this module, imported only by bench.py and tools/, applies them:

  PCD_OPT_<KEY>=<int>       pcd_set_option(<key>, <int>)                  (include/pcd_ops.h lists the keys)
  PCD_BN_FUSED_MID=0/1      ops.BN_FUSED_MID                              fold the BatchNorm mid reduction into the conv launches
  PCD_WGRAD_FLUSH_MB=<int>  spconv.functional.WGRAD_FLUSH_BYTES           slab bytes that trigger a deferred weight-gradient reduction (0: one, at the join)
  PCD_BN2D_BUMP=0/1         hotpath.conv2d_fast.BATCH_BN_COUNTERS
  PCD_RB_DEPTH=<int>        backbone3d._BackboneBase.prefetch_depth
  PCD_HOOK_AT=conv2|conv3|conv4   backbone3d._BackboneBase.after_rulebooks_at   where the after_rulebooks hook (bench.py: next batch's voxelisation) may start
  PCD_COLMAP=0/1            ops.USE_COLUMN_MAPS                           column-map rulebook builds (0: flat key-space bitmaps)
  PCD_IMPLICIT_PAIRS=0/1    ops.IMPLICIT_STRIDED_PAIRS                    strided rulebooks without indice_pairs (weight gradient over the parity classes)
  PCD_COMPACT_TABLES=0/1    ops.COMPACT_STRIDED_TABLES                    ... and with compact neighbour tables only (static plans)
"""
import os


def apply(environ=None):
    env = os.environ if environ is None else environ
    from com_amd import _lib as L, ops
    from com_amd.hotpath import backbone3d, conv2d_fast
    for k, v in env.items():
        if k.startswith("PCD_OPT_"):
            L.set_option(k[8:].lower(), int(v))                 # (raises on an unknown key)
    flag = lambda name, default: env.get(name, "1" if default else "0") != "0"
    ops.BN_FUSED_MID = flag("PCD_BN_FUSED_MID", ops.BN_FUSED_MID)
    if "PCD_WGRAD_FLUSH_MB" in env:
        from com_amd.spconv import functional as Fsp
        Fsp.WGRAD_FLUSH_BYTES = int(env["PCD_WGRAD_FLUSH_MB"]) << 20
    ops.USE_COLUMN_MAPS = flag("PCD_COLMAP", ops.USE_COLUMN_MAPS)
    ops.IMPLICIT_STRIDED_PAIRS = flag("PCD_IMPLICIT_PAIRS", ops.IMPLICIT_STRIDED_PAIRS)
    ops.COMPACT_STRIDED_TABLES = flag("PCD_COMPACT_TABLES", ops.COMPACT_STRIDED_TABLES)
    conv2d_fast.BATCH_BN_COUNTERS = flag("PCD_BN2D_BUMP", conv2d_fast.BATCH_BN_COUNTERS)
    backbone3d._BackboneBase.prefetch_depth = int(env.get("PCD_RB_DEPTH", backbone3d._BackboneBase.prefetch_depth))
    if env.get("PCD_HOOK_AT"):
        backbone3d._BackboneBase.after_rulebooks_at = None if env["PCD_HOOK_AT"] == "units" else env["PCD_HOOK_AT"]
