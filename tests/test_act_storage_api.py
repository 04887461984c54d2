"""The opt-in fp16 activation storage (isl_net_set_act_storage), CPU side: the three C entry points
are declared, listed and exported, the Python names exist, bad values are refused, the variant code
has its bit, the drop-in classes validate ``act_storage=`` at construction, and on a host without a
GPU the argument changes nothing."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from islpose import runtime as rt
from islpose import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"isl_net_set_act_storage", "isl_net_get_act_storage", "isl_net_act_storage_active"}


def _torch_weights(kind):
    return {k: torch.from_numpy(v) for k, v in synth.synth_weights(kind).items()}


def test_act_storage_symbols_declared_listed_and_exported():
    text = open(os.path.join(REPO, "include", "islpose.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(isl_\w+)\s*\(", text, re.M))
    assert SYMBOLS <= declared
    assert re.search(r"enum\s+isl_act_storage\s*\{\s*ISL_ACT_FP32\s*=\s*0\s*,\s*ISL_ACT_FP16\s*=\s*1\s*\}", text)
    assert re.search(r"#define\s+ISL_ABI_VERSION\s+1\b", text)          # additions only
    # the precision enum keeps its two values
    assert re.search(r"enum\s+isl_precision\s*\{\s*ISL_PREC_FP32\s*=\s*0\s*,\s*ISL_PREC_FP16\s*=\s*1\s*\}", text)
    assert SYMBOLS <= set(rt.EXPORTS)
    assert os.path.exists(rt.LIB_PATH), "libislpose.so not built"
    lib = ctypes.CDLL(rt.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    L = rt.lib()
    for name in SYMBOLS:
        assert getattr(L, name).argtypes is not None, name


def test_act_storage_names_and_variant_bit():
    assert rt.ACT_STORAGES == {"fp32": 0, "fp16": 1}
    assert rt.check_act_storage("fp16") == "fp16" and rt.check_act_storage(None) is None
    with pytest.raises(ValueError):
        rt.check_act_storage("bf16")
    assert rt.decode_variant(1)["act16"] is True
    assert rt.decode_variant(1 | 2 | 512)["act16"] is True
    # existing codes keep every existing key's value: the new bit adds one key and moves none
    for code in (2, 512, 1024 | 128, 1024 | 32 | 2, 4096 | 2, 32768 | 512, 65536 | (12 << 20) | (4 << 25) | (3 << 29),
                 (1 << 18) | 2 | (8 << 20) | (2 << 25) | (1 << 29), 8 | 1024, 4, 64, 16 | (4 << 25), -1, -2, 0):
        d0, d1 = rt.decode_variant(code), rt.decode_variant(code | 1) if code > 0 else rt.decode_variant(code)
        if code <= 0:
            assert "act16" not in d0
            continue
        assert d0["act16"] is False and d1["act16"] is True
        assert {k: v for k, v in d0.items() if k not in ("act16", "var")} == \
               {k: v for k, v in d1.items() if k not in ("act16", "var")}
        assert d0["var"] == code & 0xfffff and d1["var"] == d0["var"] | 1


def test_net_act_storage_roundtrip_without_device(monkeypatch):
    """isl_net_create / set / get touch no device: default fp32, the env selects fp16 at create
    time, any other value is ISL_E_ARG and an unknown name ValueError; the precision and the
    algorithm are untouched by the switch."""
    assert os.path.exists(rt.LIB_PATH), "libislpose.so not built"
    monkeypatch.delenv("ISLPOSE_ACT_STORAGE", raising=False)
    monkeypatch.delenv("ISLPOSE_PRECISION", raising=False)
    net = rt.Net(rt.ISL_BODY25)
    assert net.act_storage == "fp32" and net.act_storage_active is False
    net.set_act_storage("fp16")
    assert net.act_storage == "fp16" and net.precision == "fp32" and net.algo == "x3"
    assert net.act_storage_active is False            # nothing ran
    with net.act_storage_scope("fp32"):
        assert net.act_storage == "fp32"
    assert net.act_storage == "fp16"
    with net.algo_scope("direct"):                    # stored, kept
        assert net.act_storage == "fp16"
    net.set_precision("fp16")
    assert net.act_storage == "fp16"
    for bad in (-1, 2, 7):
        assert rt.lib().isl_net_set_act_storage(net.h, bad) == rt.ISL_E_ARG
    assert rt.lib().isl_net_set_act_storage(None, 0) == rt.ISL_E_ARG
    assert rt.lib().isl_net_get_act_storage(None) == rt.ISL_E_ARG
    assert rt.lib().isl_net_act_storage_active(None) == rt.ISL_E_ARG
    assert net.act_storage == "fp16"
    with pytest.raises(ValueError):
        net.set_act_storage("bf16")
    monkeypatch.setenv("ISLPOSE_ACT_STORAGE", "fp16")
    env = rt.Net(rt.ISL_HAND)
    assert env.act_storage == "fp16" and env.precision == "fp32"
    monkeypatch.setenv("ISLPOSE_ACT_STORAGE", "fp32")
    assert rt.Net(rt.ISL_HAND).act_storage == "fp32"
    monkeypatch.setenv("ISLPOSE_ACT_STORAGE", "half")
    assert rt.Net(rt.ISL_HAND).act_storage == "fp32"


def test_body_hand_reject_unknown_act_storage():
    """ValueError at construction, GPU or not (before the feature: TypeError, no such keyword)."""
    from src.body import Body
    from src.hand import Hand
    from islpose.body import BodyEstimator
    from islpose.hand import HandEstimator
    with pytest.raises(ValueError):
        Body(_torch_weights(0), "body25", act_storage="bogus")
    with pytest.raises(ValueError):
        Hand(_torch_weights(2), act_storage="bogus")
    with pytest.raises(ValueError):
        BodyEstimator(None, "body25", act_storage="bogus")
    with pytest.raises(ValueError):
        HandEstimator(None, act_storage="bogus")
    with pytest.raises(TypeError):          # keyword only
        Hand(_torch_weights(2), "fp16", "fp16")


def test_module_stores_act_storage_until_the_net_exists():
    from src.body import Body
    from src.ISL_Model_parameter import ISLSignPos
    from src.hand import Hand
    body = Body(_torch_weights(0), "body25", precision="fp16", act_storage="fp16")
    hand = Hand(_torch_weights(2))
    assert body.act_storage == "fp16" and body.model.act_storage == "fp16"
    assert hand.act_storage is None and hand.model.act_storage is None
    # the bits do not change with the storage: cached feature rows stay valid
    isl = ISLSignPos(body.model, hand.model)
    k0 = isl.state_key()
    hand.model.set_act_storage("fp16")
    body.model.set_act_storage("fp32")
    assert isl.state_key() == k0
    with pytest.raises(ValueError):
        body.model.set_act_storage("bogus")


@pytest.mark.skipif(torch.cuda.is_available(), reason="the CPU path of a GPU-less host")
def test_act_storage_is_accepted_and_inert_on_the_cpu_path():
    from src.body import Body
    from src.hand import Hand
    img = synth.synth_frames(1, 64, 96, seed=3)[0]
    b0 = Body(_torch_weights(0), "body25")
    b1 = Body(_torch_weights(0), "body25", precision="fp16", act_storage="fp16")
    assert b1.act_storage == "fp16" and b1.model.act_storage == "fp16"
    (c0, s0), (c1, s1) = b0(img), b1(img)
    assert np.array_equal(c0, c1) and np.array_equal(s0, s1)
    crop = synth.synth_frames(1, 48, 48, seed=4)[0]
    h0, h1 = Hand(_torch_weights(2)), Hand(_torch_weights(2), precision="fp16", act_storage="fp16")
    assert np.array_equal(h0(crop), h1(crop))
