"""Shared by the resident-dataset tests: the golden debug SID options and a synthetic LMDB set in which three short
exposures share one long frame (written with tests/sid_fixtures.py)."""
from __future__ import annotations

import json
import os

import numpy as np

from sid_fixtures import encode_png, write_lmdb

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sid")


def read_gold(rel):
    with open(os.path.join(GOLD, rel), "rb") as f:
        return f.read()


def gold_opt(**kw):
    """The options of tests/test_sid_input.py's `_opt` (golden debug LMDB, train_small, patch 24, seed 123)."""
    opt = {"manifest_path": os.path.join(GOLD, "manifest_sid_debug.json"), "phase": "train", "subset": "train_small",
           "io_backend": {"type": "lmdb", "db_paths": [os.path.join(GOLD, "train_small_short.lmdb"),
                                                        os.path.join(GOLD, "train_small_long.lmdb")],
                          "client_keys": ["short", "long"]},
           "patch_size": 24, "samples_per_pair": 5, "seed": 123}
    opt.update(kw)
    return opt


def gold_disk_backend():
    return {"type": "disk", "paths": {"short": os.path.join(GOLD, "short"), "long": os.path.join(GOLD, "long")}}


# short frames of four sizes; s0..s2 share the long frame "la", s3 has its own "lb"
SHORT_SHAPES = {"s0.png": (12, 20), "s1.png": (16, 16), "s2.png": (9, 31), "s3.png": (10, 10)}
LONG_SHAPES = {"la.png": (16, 31), "lb.png": (10, 12)}
LONG_OF = {"s0.png": "la.png", "s1.png": "la.png", "s2.png": "la.png", "s3.png": "lb.png"}


def write_shared_long_set(root, long_shapes=None, corrupt_idat=False, **kw):
    """Write the synthetic set under `root`; returns (dataset options, {("short" | "long", key): uint16 HWC array})."""
    rng = np.random.default_rng(7)
    long_shapes = dict(LONG_SHAPES, **(long_shapes or {}))
    arrays, dbs = {}, {"short": {}, "long": {}}
    for client, shapes in (("short", SHORT_SHAPES), ("long", long_shapes)):
        for key, (h, w) in shapes.items():
            a = rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)
            png = encode_png(a, 16, 2, filters=0)
            if corrupt_idat:  # IHDR stays fine; the DEFLATE stream (and the IDAT CRC) do not
                i = png.index(b"IDAT") + 10
                png = png[:i] + bytes([png[i] ^ 0x55]) + png[i + 1:]
            arrays[(client, key)] = a
            dbs[client][key.encode()] = png
    for client in ("short", "long"):
        os.makedirs(os.path.join(root, f"{client}.lmdb"), exist_ok=True)
        write_lmdb(os.path.join(root, f"{client}.lmdb", "data.mdb"), dbs[client])
    manifest = [{"pair_id": f"pair{i}", "subset": "train", "short_key": s, "long_key": LONG_OF[s],
                 "short_exposure": 0.1, "long_exposure": 10.0, "exposure_ratio": float(r)}
                for i, (s, r) in enumerate(zip(SHORT_SHAPES, (100.0, 250.0, 300.0, 100.0)))]
    with open(os.path.join(root, "manifest.json"), "w") as f:
        json.dump(manifest, f)
    opt = {"manifest_path": os.path.join(root, "manifest.json"), "phase": "train", "subset": "train",
           "io_backend": {"type": "lmdb", "db_paths": [os.path.join(root, "short.lmdb"),
                                                        os.path.join(root, "long.lmdb")],
                          "client_keys": ["short", "long"]},
           "patch_size": 8, "samples_per_pair": 2, "seed": 5}
    opt.update(kw)
    return opt, arrays
