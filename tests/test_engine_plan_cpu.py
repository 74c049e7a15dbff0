"""Host side of the inference engines that needs no GPU: the batch-part rule (engine.resolve_parts) and the public signatures of
``plan`` / ``pipeline`` / ``forward``, which bench.py, model.py and the tests call positionally."""
import inspect

import pytest

from focoos_amd.engine import DEFAULT_STREAMS, MIN_PART_BATCH, DetrEngine, resolve_parts
from focoos_amd.engine_bf import BfEngine
from focoos_amd.engine_cls import ClsEngine
from focoos_amd.engine_mf import MfEngine

# parts of a step of B images for a requested nsplit of 1, 2, 3, 4: counted down to a divisor of B that leaves every part >= 4 images
PARTS = {
    1: (1, 1, 1, 1),
    2: (1, 1, 1, 1),
    4: (1, 1, 1, 1),      # 4 / 2 = 2 < MIN_PART_BATCH
    6: (1, 1, 1, 1),      # 6 / 2 = 3 < MIN_PART_BATCH
    7: (1, 1, 1, 1),      # no divisor
    8: (1, 2, 2, 2),      # 3 does not divide 8; 8 / 4 = 2 is too small
    16: (1, 2, 2, 4),
    32: (1, 2, 2, 4),
}


def test_constants():
    assert (DEFAULT_STREAMS, MIN_PART_BATCH) == (2, 4)     # PARTS is written out for these


@pytest.mark.parametrize("B", sorted(PARTS))
def test_resolve_parts_requested(B, monkeypatch):
    monkeypatch.setenv("FX_STREAMS", "4")                  # an explicit request does not read the environment
    for nsplit, want in zip((1, 2, 3, 4), PARTS[B]):
        assert resolve_parts(B, nsplit, True) == want, (B, nsplit)
        assert resolve_parts(B, nsplit, False) == 1, (B, nsplit)


@pytest.mark.parametrize("B", sorted(PARTS))
@pytest.mark.parametrize("env", [None, "1", "3"])
def test_resolve_parts_from_environment(B, env, monkeypatch):
    if env is None:
        monkeypatch.delenv("FX_STREAMS", raising=False)
    else:
        monkeypatch.setenv("FX_STREAMS", env)
    want = PARTS[B][int(env or DEFAULT_STREAMS) - 1]
    assert resolve_parts(B, None, True) == want
    assert resolve_parts(B, None, False) == 1


def test_resolve_parts_examples():
    assert resolve_parts(8, 2, True) == 2
    assert resolve_parts(6, 2, True) == 1
    assert resolve_parts(16, 3, True) == 2
    assert resolve_parts(7, 2, True) == 1
    assert resolve_parts(32, 4, False) == 1


_REQ = inspect.Parameter.empty
_MASK = {
    "plan": [("B", _REQ), ("H", _REQ), ("W", _REQ), ("f32_input", False), ("full_masks", None), ("nsplit", None)],
    "pipeline": [("B", _REQ), ("H", _REQ), ("W", _REQ), ("depth", None), ("f32_input", False), ("nsplit", 1), ("full_masks", None)],
    "forward": [("images", _REQ), ("threshold", None), ("forced_attn", None), ("use_graph", True), ("full_masks", None)],
}
SIGNATURES = {
    DetrEngine: {
        "plan": [("B", _REQ), ("H", _REQ), ("W", _REQ), ("f32_input", False), ("nsplit", None)],
        "pipeline": [("B", _REQ), ("H", _REQ), ("W", _REQ), ("depth", None), ("f32_input", False), ("nsplit", 1)],
        "forward": [("images", _REQ), ("sizes", None), ("threshold", None), ("forced_topk", None), ("use_graph", True)],
    },
    MfEngine: _MASK,
    BfEngine: _MASK,
    ClsEngine: {
        "plan": [("B", _REQ), ("H", _REQ), ("W", _REQ), ("f32_input", False)],
        "pipeline": [("B", _REQ), ("H", _REQ), ("W", _REQ), ("depth", None), ("f32_input", False)],
        "forward": [("images", _REQ), ("use_graph", True)],
    },
}


@pytest.mark.parametrize("cls", list(SIGNATURES), ids=lambda c: c.__name__)
@pytest.mark.parametrize("method", ["plan", "pipeline", "forward"])
def test_public_signatures(cls, method):
    params = list(inspect.signature(getattr(cls, method)).parameters.values())
    assert params[0].name == "self"
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)
    assert [(p.name, p.default) for p in params[1:]] == SIGNATURES[cls][method]
