"""The inputs of test_gpu_write.py as plain data, so that test_write_host.py can walk the same clouds, writes and poses
without a GPU: `scenario(name, n)` gives a start cloud and a list of writes (selection, window, records), `replay` the
host model (write_model.Model) after each of them, `pose` the camera of a frame check (edit_model.pose_for).  numpy only."""
import numpy as np

import edit_model as em
import helpers
import write_model as wm

W, H = em.W, em.H  # 160 x 128
COUNTS = (1, 255, 256, 257, 1023, 4099, 8229)  # the chunk edges
SHAPES = ("all", "random", "point_0", "point_last", "one_chunk", "every_other_chunk", "last_partial_chunk", "empty")
BIG = (4099, 8229)  # the counts of the scenarios that need chunks behind the written span


def cloud(n, seed=3):
    xyzw, rgba = helpers.random_cloud(n, seed + n)
    return np.ascontiguousarray(xyzw[:, :3]), np.ascontiguousarray(rgba[:, :3])


def selection(shape, n, seed=5):
    idx = np.arange(n)
    last = n - n % 256 if n % 256 else n - 256
    if shape == "all":
        return None
    return {"random": np.random.default_rng(seed + n).random(n) < 0.3, "point_0": idx == 0, "point_last": idx == n - 1,
            "one_chunk": (idx >= 256) & (idx < 512), "every_other_chunk": (idx // 256) % 2 == 0,
            "last_partial_chunk": idx >= last, "empty": np.zeros(n, bool)}[shape]


def windows(k):
    """(first, count) of the writes on a selection of k points; the last two change nothing."""
    return [(0, k), (k // 3, k // 2), (0, 1), (max(k - 1, 0), 5), (k, 3), (k // 2, 0)]


def records(kind, m, seed):
    """m records: xyz float32 (m, 3), rgb uint8 (m, 3)."""
    rng = np.random.default_rng([seed, m])
    rgb = rng.integers(0, 256, (m, 3), dtype=np.uint8)
    if kind == "box":       # a box beside the start cloud's
        xyz = rng.uniform((2, -1, -3), (6, 2, 1), (m, 3)).astype(np.float32)
    elif kind == "collapse":  # every record the same point: the chunks' widths go to 0
        xyz = np.tile(np.float32([1.25, -0.5, 2.0]), (m, 1))
    elif kind == "wide":    # mixed signs on every axis, exponents 2^-6 .. 2^5: 32-bit chunks with box words
        xyz = (rng.uniform(-1, 1, (m, 3)) * 2.0 ** rng.integers(-6, 6, (m, 3))).astype(np.float32)
    elif kind == "far":     # 1000 x farther out than anything resident
        xyz = rng.uniform((2000, -1000, -3000), (6000, 2000, 1000), (m, 3)).astype(np.float32)
    elif kind == "specials":  # NaNs with payloads, +-inf, -0, denormals among ordinary values
        xyz = rng.uniform((2, -1, -3), (6, 2, 1), (m, 3)).astype(np.float32)
        hit = rng.random((m, 3)) < 0.2
        xyz[hit] = em.SPECIALS[rng.integers(0, em.SPECIALS.size, int(hit.sum()))]
    else:
        raise ValueError(kind)
    return xyz, rgb


def _step(sel, first, count, kind, streams, seed):
    X, C = records(kind, count, seed)
    return {"sel": sel, "first": first, "X": X if streams in ("xyz", "both") else None,
            "C": C if streams in ("rgb", "both") else (np.uint8([250, 40, 10]) if streams == "colour" else None),
            "kind": kind, "streams": streams}


def scenario(name, n):
    """-> (xyz, rgb, steps).  "forms:<shape>": the six windows on one selection shape, the streams in turn;
    "packed": the values that move the packed form; "specials": the special bit patterns; "pieces": a selection
    written in three pieces; "colour": one colour onto half the cloud."""
    xyz, rgb = cloud(n)
    if name.startswith("forms:"):
        sel = selection(name[6:], n)
        k = n if sel is None else int(sel.sum())
        steps = [_step(sel, f, c, "box", ("both", "xyz", "rgb", "both", "both", "xyz")[j], 10 * j + len(name))
                 for j, (f, c) in enumerate(windows(k))]
    elif name == "packed":  # (a start cloud of one sign on every axis: its chunks pack to a common prefix)
        xyzw, _ = helpers.random_cloud(n, 17 + n, (1, 1, 1), (5, 3, 5))
        xyz = np.ascontiguousarray(xyzw[:, :3])
        idx = np.arange(n)
        mid = (idx >= 256) & (idx < n - 600)  # whole chunks, with chunks resident in front of and behind them
        k = int(mid.sum())
        steps = [_step(mid, 0, k, "collapse", "xyz", 1),           # widths to 0: the tail's blocks move down
                 _step(None, 0, n, "wide", "both", 2),             # every chunk wide: the planes outgrow their capacity
                 _step(mid, 0, k, "collapse", "xyz", 3),           # ... and shrink by more than 1/8: reallocated
                 _step(idx >= n - n // 5, 0, n // 5, "far", "xyz", 4)]  # the lane test's absmax must follow
    elif name == "specials":
        sel = selection("random", n)
        steps = [_step(sel, 0, int(sel.sum()), "specials", "both", 7), _step(None, n // 2, n // 4, "specials", "xyz", 8)]
    elif name == "pieces":
        sel = selection("random", n)
        k = int(sel.sum())
        X, C = records("box", k, 9)
        cuts = [0, k // 3, k // 3 + max(1, k // 4), k]
        steps = [{"sel": sel, "first": a, "X": X[a:b], "C": C[a:b], "kind": "box", "streams": "both"} for a, b in zip(cuts, cuts[1:])]
    elif name == "colour":
        steps = [_step(np.arange(n) % 2 == 0, 0, 0, "box", "colour", 0), _step(None, n // 3, 0, "box", "colour", 0)]
    else:
        raise ValueError(name)
    return xyz, rgb, steps


def names(n):
    out = ["forms:" + s for s in SHAPES] + ["specials", "pieces", "colour"]
    return out + ["packed"] if n in BIG else out


def replay(name, n):
    """[(step, model after it)] on the host model."""
    xyz, rgb, steps = scenario(name, n)
    model = wm.Model("pack2_ids")
    model.upload(xyz, rgb)
    out = []
    for st in steps:
        model.write(st["sel"], st["first"], st["X"], st["C"])
        out.append((st, model.copy()))
    return out


def pose(model, k):
    return em.pose_for(model, k)
