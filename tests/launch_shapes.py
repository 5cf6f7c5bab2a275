"""The launch shape a batch takes, asked of the library (hkv_debug_launch_shape:
the plan of haskoin-node_amd/csrc/hkv_launch_plan.h, the one the verify entry
points run on), for GPU tests that mean a particular shape."""
import ctypes

BLOCK, PAIR, MID, TABLE_CHAIN = 1, 2, 3, 4          # hkv::Shape
SCAN_IN_KERNEL, ROWS_IN_KERNEL, OVERLAP = 1, 2, 4   # the standard-input flags


def _query(ver, kind, n):
    out = (ctypes.c_uint32 * 4)()
    assert ver.lib.hkv_debug_launch_shape(ver.ctx, 0, kind, n, out) == 0
    return tuple(out)


def records(ver, n):
    """(shape, 0, first chunk's length, chunks) of a batch of n records on device 0."""
    return _query(ver, 0, n)


def std_inputs(ver, n):
    """(first chunk's shape, its flags, its length, chunks) of a batch of n standard inputs on device 0."""
    return _query(ver, 1, n)
