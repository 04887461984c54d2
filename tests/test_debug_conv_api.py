"""isl_debug_conv's descriptor checks, which run before any device work (no GPU here): malformed
descriptors and shapes the named kernel does not take are ISL_E_ARG."""
import ctypes
import os

import numpy as np
import pytest

from islpose import runtime as rt


def test_library_is_built():
    assert os.path.exists(rt.LIB_PATH), "libislpose.so not built (make, or __graft_entry__.build())"


def _layer(cin=16, cout=26, ks=3, n=1, h=9, w=13):
    return (np.zeros((n, cin, h, w), np.float32), np.zeros((cout, cin, ks, ks), np.float32), np.zeros(cout, np.float32))


def _arg_error(*a, **kw):
    with pytest.raises(rt.IslError, match=r"\(-1\)"):
        rt.debug_conv(*a, **kw)


def test_struct_sizes_match_the_header():
    assert ctypes.sizeof(rt.IslDebugConvDesc) == 4 * (18 + 12 + 3 + 7)
    assert ctypes.sizeof(rt.IslDebugConvResult) == 8 + 16 + 4 * 12


def test_descriptor_checks():
    x, wt, b = _layer()
    _arg_error(x, wt, b, act16=True)                                   # act16 needs f16
    _arg_error(x, wt, b, in_pad=2)                                     # rings are 1 or 3
    _arg_error(x, wt, b, out_pad=0)
    _arg_error(x, wt, b, in_coff=4)                                    # slices on chunks
    _arg_error(x, wt, b, out_coff=8, out_cs=32)                        # the slice leaves the buffer
    _arg_error(x, wt, b, segs=[(0, 0, 8), (4, 8, 8)])                  # segments overlap physically
    _arg_error(x, wt, b, segs=[(0, 0, 8)])                             # a logical channel without a segment
    _arg_error(x, wt, b, kernel="direct", f16=True)                    # f16 is a form of x3 / rgb
    _arg_error(x, wt, b, kernel="wino2")                               # cout % 64
    _arg_error(x, wt, b, kernel="wino")                                # cout fits no Winograd tile
    _arg_error(x, wt, b, kernel="rgb")                                 # cin != 3
    _arg_error(x, wt, b, hpool=True)                                   # odd width
    _arg_error(x, wt, b, kernel="direct", allow_split=True)            # conv_x3's switch
    x7, w7, b7 = _layer(ks=7)
    _arg_error(x7, w7, b7, in_pad=1)                                   # ring narrower than the radius
    with pytest.raises(ValueError):
        rt.debug_conv(x, wt, b, act="prelu")                           # no slopes
    with pytest.raises(ValueError):
        rt.debug_conv(x, wt[:, :8], b)


def test_reserved_fields_must_be_zero():
    x, wt, b = _layer()
    d = rt.IslDebugConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ks = 1, 9, 13, 16, 26, 3
    d.in_pad = d.out_pad = 1
    d.in_cs, d.out_cs, d.nseg = 16, 32, 1
    d.seg[0] = rt.IslDebugSeg(0, 0, 16)
    d.reserved[3] = 1
    y = np.empty((1, 26, 9, 13), np.float32)
    r = rt.IslDebugConvResult()
    rc = rt.lib().isl_debug_conv(ctypes.byref(d), x.ctypes.data, wt.ctypes.data, b.ctypes.data, None, y.ctypes.data,
                                 None, ctypes.byref(r))
    assert rc == rt.ISL_E_ARG
    assert rt.lib().isl_debug_conv(None, x.ctypes.data, wt.ctypes.data, b.ctypes.data, None, y.ctypes.data, None,
                                   ctypes.byref(r)) == rt.ISL_E_ARG


def test_oversized_call_is_an_argument_error():
    """A descriptor within the per-field limits whose buffers pass 256 MiB is ISL_E_ARG before
    anything is allocated or read (the array pointers are never followed)."""
    d = rt.IslDebugConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ks = 256, 1024, 1024, 16, 26, 3
    d.in_pad = d.out_pad = 1
    d.in_cs, d.out_cs, d.nseg = 16, 32, 1
    d.seg[0] = rt.IslDebugSeg(0, 0, 16)
    dummy = np.zeros(16, np.float32)
    r = rt.IslDebugConvResult()
    rc = rt.lib().isl_debug_conv(ctypes.byref(d), dummy.ctypes.data, dummy.ctypes.data, dummy.ctypes.data, None,
                                 dummy.ctypes.data, None, ctypes.byref(r))
    assert rc == rt.ISL_E_ARG
    # input 205 MB, pair-max buffer 102 MB, but the pooled buffer with its ring of 3: 358 MB
    d.hpool, d.n, d.h, d.w, d.out_pad = 1, 2, 2, 400000, 3
    assert rt.lib().isl_debug_conv(ctypes.byref(d), dummy.ctypes.data, dummy.ctypes.data, dummy.ctypes.data, None,
                                   dummy.ctypes.data, dummy.ctypes.data, ctypes.byref(r)) == rt.ISL_E_ARG
