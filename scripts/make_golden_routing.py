#!/usr/bin/env python
"""Generate tests/golden/conv_routing.json: the (return code, label) fx_conv2d_variant gives for a fixed grid of fx_conv_desc - the
convolution routing table of the library, recorded so that a change of the routing code that is not meant to move a layer is checked
against it (tests/test_host_cpu.py::test_conv_routing_matches_golden_census).  Host logic only: no GPU, no launch.

The grid: KH 1 / 3 x stride 1 / 2 x C x N from 32 to 2048 x output-pixel counts on both sides of the routing thresholds (5 000, 16 384,
20 000, 40 000) with W up to 400; per point the epilogue (act x residual with residual_after_act 0 / 1 / 2), with and without a
fragment-order weight copy, and out_f32, pool2, mask, y_batch_stride one at a time.  Recorded twice: with every FX_* variable unset, and
with FX_CONV3_MIN_M = FX_PW_MIN_M = 0 (the kernel tests' setting; the library re-reads these two per call, every other knob once per
process, so the script refuses to run with any other FX_* variable set).
    python scripts/make_golden_routing.py
"""
from __future__ import annotations

import ctypes as C
import json
import os
import string
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_routing.json")
GEOMS = [(1, 1), (3, 1), (1, 2), (3, 2)]                  # (KH = KW, stride)
CS = [32, 64, 128, 256, 512, 1024, 2048]
NS = [32, 64, 128, 256, 384, 512, 2048]
SHAPES = [                                                # (B, H, W): M = B * H * W at stride 1
    (800, 1, 1), (2, 16, 16), (3, 40, 40), (2, 50, 50), (10, 40, 40), (1, 128, 128), (42, 20, 20), (2, 100, 100),
    (51, 20, 20), (1, 98, 400), (1, 200, 200), (16, 80, 80), (1, 320, 320),
]
# (act, residual_after_act or None, frag, out_f32, pool2, mask, y_batch_stride)
VARIANTS = ([(act, res, 1, 0, 0, 0, 0) for act in ("none", "relu", "silu") for res in (None, 0, 1, 2)]
            + [("relu", None, 0, 0, 0, 0, 0), ("relu", None, 1, 1, 0, 0, 0), ("relu", None, 1, 0, 1, 0, 0), ("none", None, 1, 0, 0, 1, 0),
               ("relu", None, 1, 0, 0, 0, 1)])
ENVS = {"default": {}, "min_m_0": {"FX_CONV3_MIN_M": "0", "FX_PW_MIN_M": "0"}}
THRESHOLDS = ("FX_CONV3_MIN_M", "FX_PW_MIN_M")
# one character per outcome in the recorded strings (no JSON escapes)
ALPHABET = "".join(c for c in string.ascii_letters + string.digits + string.punctuation if c not in "\"\\")


def grid():
    return {"geoms": GEOMS, "C": CS, "N": NS, "shapes": SHAPES, "variants": VARIANTS}


def _desc(B, H, W, Cc, N, k, stride, act, res, frag, out_f32, pool2, mask, ybs):
    from focoos_amd._lib import FX_ACT, FxConvDesc

    d = FxConvDesc()
    pad = (k - 1) // 2
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if pool2 else ((H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1)
    ld = (N + 7) // 8 * 8
    d.x, d.w, d.y, d.bias = 0x10000, 0x20000, 0x30000, 0x40000
    d.w_frag = 0x50000 if frag else None
    d.residual = 0x60000 if res is not None else None
    d.mask, d.ldm = (0x70000, ld) if mask else (None, 0)
    d.B, d.H, d.W, d.C, d.ldx = B, H, W, Cc, Cc
    d.Ho, d.Wo, d.N, d.ldy, d.ldr = Ho, Wo, N, ld, ld if res is not None else 0
    d.KH, d.KW, d.stride, d.pad, d.pool2 = k, k, stride, pad, pool2
    d.act, d.out_f32, d.residual_after_act = FX_ACT[act], out_f32, res or 0
    d.y_batch_stride = (Ho * Wo + 8) * ld if ybs else 0
    return d


def census(lib) -> dict:
    """{env: [outcome per grid point]} in grid order (geom, C, N, shape, variant); an outcome is the label or "rc <code>"."""
    buf = C.create_string_buffer(64)
    saved = {k: os.environ.get(k) for k in THRESHOLDS}
    out = {}
    try:
        for env, setting in ENVS.items():
            for k in THRESHOLDS:
                os.environ.pop(k, None)
            os.environ.update(setting)
            rows = []
            for k, stride in GEOMS:
                for Cc in CS:
                    for N in NS:
                        for B, H, W in SHAPES:
                            for v in VARIANTS:
                                rc = lib.fx_conv2d_variant(C.byref(_desc(B, H, W, Cc, N, k, stride, *v)), buf, 64)
                                rows.append(buf.value.decode() if rc == 0 else f"rc {rc}")
            out[env] = rows
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


def points():
    """The grid points in census order, for messages: (KH, stride, C, N, (B, H, W), variant)."""
    return [(k, s, Cc, N, sh, v) for k, s in GEOMS for Cc in CS for N in NS for sh in SHAPES for v in VARIANTS]


def encode(rows_by_env: dict) -> dict:
    legend = sorted({o for rows in rows_by_env.values() for o in rows})
    assert len(legend) <= len(ALPHABET), len(legend)
    code = {o: ALPHABET[i] for i, o in enumerate(legend)}
    per_line = len(SHAPES) * len(VARIANTS)   # one line per (geom, C, N)
    enc = {}
    for env, rows in rows_by_env.items():
        s = "".join(code[o] for o in rows)
        enc[env] = [s[i:i + per_line] for i in range(0, len(s), per_line)]
    return {"legend": {code[o]: o for o in legend}, "census": enc}


def decode(doc: dict) -> dict:
    legend = doc["legend"]
    return {env: [legend[c] for c in "".join(lines)] for env, lines in doc["census"].items()}


def main():
    stray = sorted(k for k in os.environ if k.startswith("FX_") and k not in ("FX_BUILD_JOBS",))
    if stray:
        sys.exit(f"unset {stray} first: the census records the default routing")
    import torch  # noqa: F401  (HIP runtime first, see focoos_amd/_lib.py)

    from focoos_amd import _lib, build

    build.build(force=False, verbose=False)
    doc = {"doc": "fx_conv2d_variant over the grid of scripts/make_golden_routing.py; legend: character -> label or return code",
           "grid": grid(), **encode(census(_lib.load()))}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(points())} points x {len(ENVS)} settings, {len(doc['legend'])} outcomes, {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
