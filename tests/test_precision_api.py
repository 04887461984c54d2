"""The opt-in fp16 precision mode, CPU side: the two C entry points are declared and exported,
the Python names exist, the drop-in classes validate ``precision=`` at construction, and on a
host without a GPU the argument changes nothing (the CPU path is fp32)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from islpose import runtime as rt
from islpose import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_weights(kind):
    return {k: torch.from_numpy(v) for k, v in synth.synth_weights(kind).items()}


def test_precision_symbols_declared_and_exported():
    """As test_abi.py::test_header_symbols_are_exported, for the two new entries."""
    text = open(os.path.join(REPO, "include", "islpose.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(isl_\w+)\s*\(", text, re.M))
    assert {"isl_net_set_precision", "isl_net_get_precision"} <= declared
    assert re.search(r"enum\s+isl_precision\s*\{\s*ISL_PREC_FP32\s*=\s*0\s*,\s*ISL_PREC_FP16\s*=\s*1\s*\}", text)
    assert re.search(r"#define\s+ISL_ABI_VERSION\s+1\b", text)          # additions only
    assert {"isl_net_set_precision", "isl_net_get_precision"} <= set(rt.EXPORTS)
    if not os.path.exists(rt.LIB_PATH):
        pytest.skip("libislpose.so not built")
    lib = ctypes.CDLL(rt.LIB_PATH)
    assert hasattr(lib, "isl_net_set_precision") and hasattr(lib, "isl_net_get_precision")


def test_precision_names_and_variant_bit():
    assert rt.PRECISIONS == {"fp32": 0, "fp16": 1}
    # the one-term bit of isl_net_op_info's variant code.  (128 is the VAR bit of the deep-prefetch
    # loop, which the fp32 plan reports and test_gpu_body / test_gpu_hand read; the mode has bit 2)
    assert rt.decode_variant(2)["f16"] is True
    assert rt.decode_variant(512)["f16"] is False
    assert rt.decode_variant(1024 | 128)["f16"] is False


def test_net_precision_roundtrip_without_device(monkeypatch):
    """isl_net_create / set / get touch no device: default fp32, the env selects fp16 at create
    time, any other value is ISL_E_ARG and an unknown name ValueError."""
    if not os.path.exists(rt.LIB_PATH):
        pytest.skip("libislpose.so not built")
    monkeypatch.delenv("ISLPOSE_PRECISION", raising=False)
    net = rt.Net(rt.ISL_BODY25)
    assert net.precision == "fp32"
    net.set_precision("fp16")
    assert net.precision == "fp16" and net.algo == "x3"
    with net.precision_scope("fp32"):
        assert net.precision == "fp32"
    assert net.precision == "fp16"
    with net.algo_scope("direct"):          # orthogonal to the algorithm: stored, kept
        assert net.precision == "fp16"
    assert net.precision == "fp16"
    for bad in (-1, 2, 7):
        assert rt.lib().isl_net_set_precision(net.h, bad) == rt.ISL_E_ARG
    assert rt.lib().isl_net_set_precision(None, 0) == rt.ISL_E_ARG
    assert net.precision == "fp16"
    with pytest.raises(ValueError):
        net.set_precision("bf16")
    monkeypatch.setenv("ISLPOSE_PRECISION", "fp16")
    assert rt.Net(rt.ISL_HAND).precision == "fp16"
    monkeypatch.setenv("ISLPOSE_PRECISION", "fp32")
    assert rt.Net(rt.ISL_HAND).precision == "fp32"


def test_body_hand_reject_unknown_precision():
    """ValueError at construction, GPU or not (before the feature: TypeError, no such keyword)."""
    from src.body import Body
    from src.hand import Hand
    with pytest.raises(ValueError):
        Body(_torch_weights(0), "body25", precision="bogus")
    with pytest.raises(ValueError):
        Hand(_torch_weights(2), precision="bogus")
    with pytest.raises(TypeError):          # keyword only, after the reference's positionals
        Body(_torch_weights(0), "body25", "fp16")


@pytest.mark.skipif(torch.cuda.is_available(), reason="the CPU path of a GPU-less host")
def test_precision_fp16_is_accepted_and_inert_on_the_cpu_path():
    from src.body import Body
    from src.hand import Hand
    img = synth.synth_frames(1, 64, 96, seed=3)[0]
    b32, b16 = Body(_torch_weights(0), "body25"), Body(_torch_weights(0), "body25", precision="fp16")
    assert b16.precision == "fp16" and b16.model.precision == "fp16"
    (c0, s0), (c1, s1) = b32(img), b16(img)
    assert np.array_equal(c0, c1) and np.array_equal(s0, s1)
    crop = synth.synth_frames(1, 48, 48, seed=4)[0]
    h32, h16 = Hand(_torch_weights(2)), Hand(_torch_weights(2), precision="fp16")
    assert np.array_equal(h32(crop), h16(crop))


def test_state_key_follows_module_precision():
    """ISLSignPos.state_key() carries each module's precision (no device needed to set it)."""
    from src.ISL_Model_parameter import ISLSignPos
    from src.body import Body
    from src.hand import Hand
    body, hand = Body(_torch_weights(0), "body25"), Hand(_torch_weights(2))
    isl = ISLSignPos(body.model, hand.model)
    k0 = isl.state_key()
    hand.model.set_precision("fp16")
    k1 = isl.state_key()
    body.model.set_precision("fp16")
    k2 = isl.state_key()
    assert len({k0, k1, k2}) == 3
    body.model.set_precision(None)
    hand.model.set_precision(None)
    assert isl.state_key() == k0
