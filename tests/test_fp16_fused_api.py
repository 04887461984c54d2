"""Host-side checks of the fp16 mode's fused launches that need no GPU: the variant codes the plan
reports for them decode to the keys the GPU tests read.  (The hi-only packs of the fused pair are
built in the library at the first fp16 run, on the device; their layout is held by the GPU tests'
bit equality of the fused launch and its permuted two-launch form, which read different packs.)"""
from islpose import runtime as rt

X3V_A16, X3V_F16, X3V_C12, X3V_FUSE67, X3V_RGB = 1, 2, 4, 16, 1 << 18


def _code(var, ks, bpx, bco):
    """internal.h's x3_variant_code."""
    return (var & 0xfffff) | ((bpx // 32) << 20) | ((bco // 32) << 25) | ((ks // 2) << 29)


def test_decode_c12_one_term():
    for a16 in (0, 1):
        d = rt.decode_variant(_code(X3V_C12 | X3V_F16 | X3V_RGB | (X3V_A16 if a16 else 0), 3, 256, 64))
        assert d["c12"] and d["f16"] and d["rgb"] and d["act16"] == bool(a16)
        assert (d["ks"], d["bpx"], d["bco"]) == (3, 256, 64)
        assert not d["fused67"] and not d["wave_ranges"] and not d["wino2"]
    d32 = rt.decode_variant(_code(X3V_C12, 3, 256, 64))          # the fp32 plan's code, unchanged
    assert d32["c12"] and not d32["f16"] and not d32["act16"] and not d32["rgb"]


def test_decode_fused_pair_one_term():
    # the fused pair records its all-channel tile halved; decode_variant doubles it back
    for cout6, bpx in ((512, 128), (256, 256), (128, 512)):
        for extra in (0, X3V_F16, X3V_F16 | X3V_A16):
            d = rt.decode_variant(_code(X3V_FUSE67 | extra, 1, bpx, cout6 // 2))
            assert d["fused67"] and d["ks"] == 1 and d["bco"] == cout6 and d["bpx"] == bpx
            assert d["f16"] == bool(extra & X3V_F16) and d["act16"] == bool(extra & X3V_A16)
            assert not d["c12"] and not d["rgb"] and not d["ranged"] and not d["split"]


def test_decode_swallowed_ops():
    assert rt.decode_variant(-2) == {"fused_into_prev": True}
    assert rt.decode_variant(-1) == {"pool_fused": True}
    assert rt.decode_variant(0) == {}
