"""rows_model.py with the scan registration and the smooth segments in it (include/rtr_register.h section 6p,
include/rtr_segments.h section 6q): `Model` gains `segments`, `register`, `register_loop` (ProjectCloud.registerPoints)
and `remove_small_segments` (ProjectCloud.removeSmallSegments), the sequences gain their steps among the appends,
removals, moves, masks, selections, sorts and writes write_model draws -- so that rtr_select_segments, which gathers one
normal per resident position from arrays in upload order and labels a segment by its smallest upload index, and
rtr_register_points, which extracts the winners chunk by chunk and reads normals[3 * winner], run on clouds that edits
have rewritten in place and whose indices removals have renumbered.  test_gpu_surface_sequences.py drives the library
with them, test_surface_model_host.py checks this file without a GPU.  numpy only.

Results come from the existing references alone and no arithmetic is added: segments_ref.labels_brute (up to 4096
points; above, segments_ref.edges and clusters_ref.labels_of_pairs) with clusters_ref's hits, stats and words and
select_ref.combine; register_ref.register and register_ref.loop with nearest_ref.nearest_brute as the finder;
normals_ref.estimate through rows_model.Model.normals; analysis_model.beyond_span predicts RTR_ERR_UNSUPPORTED -- for a
registration on the POSED given points.

Records.  "call" = "surface"; "kind": "segments", "register", "register_loop" or "remove_small_segments"; "radius";
"edge": None, "beyond_span", "at_span", "pose_span" or the name of the directed step; "state": nearest_model's.
The normals and the curvature of a step are named by their SOURCE, never by value: "source" = "estimated"
(normals_ref.estimate on the current cloud at the record's "k" and "nradius"; "held": the arrays are the very ones the
sequence's last normals step wrote), "indexed" (`indexed`: one of four unit directions by upload index, a curvature in
[0, 0.04) from a hash of the index and n) or "constant" (one direction, no curvature); "where": the caller's arrays lie
in "host" or "device" memory.
segments: "cos_angle", "max_curvature" (None: no curvature is passed), "min_points", "max_points", "oriented", "seeded",
"op", "outside", "labels" ("host", "device" or None: NULL), "stats" (False: NULL).
register: "ask" (the outputs that are no NULL pointers, of "moments", "step" and "stats"), "plane", "pose" (None or 12 floats), "given": the spec of the given points (`scan`) -- resident points taken at
a stride of 16 from a "part" of the cloud and moved BACK by "motion" (16 floats, register_cases' recipe: 2 degrees about
(1, 2, 3) and a shift, about the centre of the chosen points and in units of their spacing), {"ref": i}: the given
points of step i of the same sequence --, "rows": "host" or "device", "width": 3 or 4 floats per row.
register_loop: register's with "iterations".  remove_small_segments: "k", "angle", "max_curvature", "min_points".
Every other record is rows_model's."""
import functools
import math

import numpy as np

import analysis_model as am
import clusters_ref as cr
import edit_model as em
import nearest_model as nm
import nearest_ref
import register_ref as rr
import rows_model as rm
import segments_ref as sg
import select_ref
import write_model as wm
from analysis_model import FAMILIES, axis_in_span, beyond_span, pose_for  # noqa: F401
from rows_model import MAX_PAIRS

f32, f64 = np.float32, np.float64
SEEDS = (1, 2, 3)
STEPS = 30
KINDS = ("segments", "register", "register_loop", "remove_small_segments")
CALLS = ("segments", "register")
SOURCES = ("indexed", "estimated", "constant")
DIRS = f32([[0, 0, 1], [0, 0, -1], [0, 1, 0], [1, 0, 0]])  # (test_gpu_segments.py's: three classes by |dot|, four by dot)
CONSTANT = f32([0.6, 0, -0.8])
COMBINING = rm.COMBINING
SHARED = nm.SHARED
EMPTY_APPEND = nm.EMPTY_APPEND
GIVEN_ROTATION = nm.GIVEN_ROTATION
PLACES = ("host", "device", None)
BRUTE_MAX = 4096   # (segments_ref.labels_brute up to here, the pair list above)
STRIDE = 16        # (register_cases.SCENE_STRIDE: every 16th point is a given point)
HEAVY = ("ties", "pipeline", "seeded")  # (the long chains: each in one sequence of a family, see _Gen)
SPAN = ("beyond_span", "at_span", "pose_span")
ASKS = (("moments", "step", "stats"), ("moments", "stats"), ("moments", "step", "stats"), ("step",))  # (each may be NULL)
# the seeded chain's (op, outside, oriented) by family -- one sequence of a family holds the chain, six in all: every
# combining op, add and toggle with and without outside, each value of oriented three times
SEEDED = (("add", True, False), ("subtract", False, True), ("intersect", True, True), ("toggle", False, False), ("add", False, True),
          ("toggle", True, False))
DIRECTED_TRIVIAL = ("degenerate_plane", "degenerate_point", "no_pair")  # (directed steps that are trivial on purpose)


# ---- the inputs a record names ------------------------------------------------------------------------------------------
def indexed(n):
    """(normals (n, 3), curvature (n,)) float32: a function of the upload index u and n alone.  DIRS[(u + u // 16) % 4]
    (plain u % 4 is ONE direction on every 16th point, which is what the given points are taken from), and a curvature
    in [0, 0.04) from a multiplicative hash of u and n -- two points that coincide still differ in both."""
    u = np.arange(n, dtype=np.uint64)
    h = (u * np.uint64(2654435761) + np.uint64(n) * np.uint64(40503)) % np.uint64(1 << 32)
    curv = ((h >> np.uint64(8)).astype(f64) / 2.0 ** 24 * 0.04).astype(f32)
    return np.ascontiguousarray(DIRS[((u + u // np.uint64(STRIDE)) % np.uint64(4)).astype(np.int64)]), curv


def motion(centre, spacing, extent, part=1.0, shift=1.2):
    """register_cases.rigid about `centre`: `part` of 2 degrees -- of the angle that moves a point `extent` away by 1.5
    spacings, where that is less: an edit may have thrown half the cloud a thousand radii away -- about (1, 2, 3), then
    `shift` spacings along (2, -2, 1) / 3."""
    a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    t = part * min(math.radians(2.0), 1.5 * spacing / extent if extent > 0 else 1.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = np.asarray(centre, f64) - R @ np.asarray(centre, f64) + shift * spacing * np.array([2.0, -2.0, 1.0]) / 3.0
    return M


def chosen(g, model):
    """Upload indices of the resident points a given-points spec names: the finite points of its part, every STRIDE-th
    from a start the seed names, then the next start, ... -- as many as "count" asks for, again from the front where
    the part holds fewer."""
    n = model.n
    if "indices" in g:  # (the ties' originals, by name)
        return np.array(g["indices"], np.int64)
    fin = np.flatnonzero(np.isfinite(model.xyz).all(axis=1))
    part = g["part"]
    if part == "first_chunk":
        fin = fin[fin < em.CHUNK]
    elif part == "last_chunk":
        fin = fin[fin >= em.CHUNK * ((n - 1) // em.CHUNK)]
    elif isinstance(part, list):
        fin = fin[(fin >= part[0]) & (fin < part[1])]
    elif isinstance(part, dict):  # (the points of one box: one part of a cloud whose parts edits have scaled apart)
        q = model.xyz[fin].astype(f64)
        fin = fin[((q >= np.array(part["lo"])) & (q <= np.array(part["hi"]))).all(axis=1)]
    if g["count"] == 0 or fin.size == 0:
        return np.zeros(0, np.int64)
    order = np.concatenate([fin[(g["seed"] + s) % STRIDE::STRIDE] for s in range(STRIDE)])
    return np.resize(order, g["count"])


def scan(rec, model, past=None):
    """float32 (m, 3): the given points of a register record on the model's state before the step."""
    g = rec["given"]
    if "ref" in g:
        return past[g["ref"]]["G"]
    p = model.xyz[chosen(g, model)]
    if g["motion"] is not None:
        with np.errstate(all="ignore"):
            p = rr_unmoved(p, np.array(g["motion"], f64).reshape(4, 4))
    G = np.ascontiguousarray(p, f32).reshape(-1, 3).copy()
    rng = np.random.default_rng(g["seed"])
    for s in range(min(g["specials"], G.shape[0])):
        G[rng.integers(G.shape[0]), rng.integers(3)] = em.SPECIALS[rng.integers(em.SPECIALS.size)]
    return G


def rr_unmoved(points, M):
    """register_cases.unmoved: the points whose image under M is `points`, M^-1 in float64, rounded to float32."""
    Mi = np.linalg.inv(M)
    return (points.astype(f64) @ Mi[:3, :3].T + Mi[:3, 3]).astype(f32)


# ---- the labels, computed once per (cloud, relation) --------------------------------------------------------------------
_LABELS = {}


def _key(*arrays):
    return tuple(None if a is None else (a.shape, hash(np.ascontiguousarray(a).tobytes())) for a in arrays)


# ---- the model ----------------------------------------------------------------------------------------------------------
class Model(rm.Model):
    """rows_model.Model with the two calls and their two facade loops.  Each returns a dict: "error" (None or
    "unsupported": the facade raises RtrError with RTR_ERR_UNSUPPORTED and nothing changes) and the call's outputs."""

    def copy(self):
        m = Model(self.family)
        m.__dict__.update(em.Model.copy(self).__dict__)
        return m

    def inputs(self, rec):
        """(normals, curvature) of a record's source on this cloud; curvature None for "constant"."""
        if rec["source"] == "indexed":
            return indexed(self.n)
        if rec["source"] == "constant":
            return np.ascontiguousarray(np.tile(CONSTANT, (self.n, 1))), None
        e = self.normals(rec["k"], rec["nradius"])
        return (None, None) if e["error"] else (e["normals"], e["curvature"])

    def labels(self, radius, cos_angle, normals, curvature=None, max_curvature=np.inf, oriented=False):
        key = _key(self.xyz, normals, curvature) + (float(radius), float(cos_angle), float(max_curvature), bool(oriented))
        lab = _LABELS.get(key)
        if lab is None:
            if len(_LABELS) >= 6:
                _LABELS.pop(next(iter(_LABELS)))
            if self.n <= BRUTE_MAX:
                lab = sg.labels_brute(self.xyz, radius, cos_angle, normals, curvature, max_curvature, oriented)
            else:
                lab = cr.labels_of_pairs(self.n, *sg.edges(self.xyz, radius, cos_angle, normals, curvature, max_curvature, oriented))
            _LABELS[key] = lab
        return lab

    def segments(self, radius, cos_angle, normals, curvature=None, max_curvature=np.inf, min_points=1, max_points=0,
                 oriented=False, seeded=False, op="replace", outside=False):
        assert self.n > 0
        if beyond_span(self.xyz, radius).any():
            return {"error": "unsupported"}
        lab = self.labels(radius, cos_angle, normals, curvature, max_curvature, oriented)
        seeds = None
        if seeded:
            seeds = np.zeros(self.n, bool) if self.selection is None else self.selection
        hit = sg.hits(lab, min_points, max_points, seeds)
        st = sg.stats(lab, hit)
        return {"error": None, "hit": hit, "labels": lab, "stats": (self._combine(op, outside, hit),) + tuple(st),
                "selection": self.selection.copy()}

    def register(self, G, radius, plane=False, pose=None, normals=None, finder=nearest_ref.nearest_brute):
        """Reads and changes nothing of the model."""
        assert self.n > 0
        with np.errstate(all="ignore"):
            P = rr.posed(G, pose)
        if beyond_span(P, radius).any():
            return {"error": "unsupported"}
        with np.errstate(all="ignore"):
            mom, step, st = rr.register(self.xyz, G, radius, rr.POINT_TO_PLANE if plane else 0, pose, normals if plane else None, finder)
        return {"error": None, "moments": mom, "step": step, "stats": tuple(int(v) for v in st)}

    def register_loop(self, G, radius, iterations, plane=False, normals=None, pose=None):
        """ProjectCloud.registerPoints.  (A later pose of the loop that carried a point beyond the span would make the
        facade raise in mid-loop: the generator draws no such loop, and this says so.)"""
        assert self.n > 0
        with np.errstate(all="ignore"):
            if beyond_span(rr.posed(G, pose), radius).any():
                return {"error": "unsupported"}
            out, rms, st = rr.loop(self.xyz, G, radius, iterations, plane, normals if plane else None, pose, nearest_ref.nearest_brute)
            assert not beyond_span(rr.posed(G, out[:3]), radius).any()
        return {"error": None, "pose": out, "rms": [float(v) for v in rms], "stats": tuple(int(v) for v in st)}

    def remove_small_segments(self, radius, k, angle, max_curvature, min_points):
        """ProjectCloud.removeSmallSegments: normals at (k, radius), the segments of min_points or more, everything else
        goes through the model's own removal, as rows_model.Model.cleanup removes."""
        assert self.n > 0
        if beyond_span(self.xyz, radius).any():
            return {"error": "unsupported"}
        e = self.normals(k, radius)
        cos_angle = f32(math.cos(float(angle)))
        hit = self.copy().segments(radius, cos_angle, e["normals"], e["curvature"], max_curvature, min_points)["hit"]
        self.remove(hit)
        return {"error": None, "hit": hit, "removed": int((~hit).sum())}


# ---- step records ---------------------------------------------------------------------------------------------------------
def materialize(rec, model, past=None):
    if rec["call"] != "surface":
        return rm.materialize(rec, model, past)
    kind, out = rec["kind"], {}
    if kind == "remove_small_segments":
        return out
    if kind == "segments" or rec["plane"]:
        out["normals"], out["curvature"] = model.inputs(rec)
    if kind != "segments":
        out["G"] = scan(rec, model, past)
        out["pose"] = None if rec["pose"] is None else np.array(rec["pose"], f64)
    return out


def apply(model, rec, args):
    """-> the result of a surface or rows step, None for every other call."""
    if rec["call"] != "surface":
        return rm.apply(model, rec, args)
    kind = rec["kind"]
    if kind == "remove_small_segments":
        return model.remove_small_segments(rec["radius"], rec["k"], rec["angle"], rec["max_curvature"], rec["min_points"])
    if kind == "segments":
        if args["normals"] is None:  # (the normals' own radius is beyond the span: the estimate is refused already)
            return {"error": "unsupported"}
        lim = rec["max_curvature"]
        return model.segments(rec["radius"], rec["cos_angle"], args["normals"], None if lim is None else args["curvature"],
                              np.inf if lim is None else lim, rec["min_points"], rec["max_points"], rec["oriented"], rec["seeded"],
                              rec["op"], rec["outside"])
    if rec["plane"] and args["normals"] is None:
        return {"error": "unsupported"}
    if kind == "register":
        return model.register(args["G"], rec["radius"], rec["plane"], args["pose"], args.get("normals"))
    return model.register_loop(args["G"], rec["radius"], rec["iterations"], rec["plane"], args.get("normals"), args["pose"])


def advance(model, rec, res):
    """What a surface or rows step does to the model, from the result `apply` gave on a copy: nothing is computed again."""
    if rec["call"] == "rows":
        return rm.advance(model, rec, res)
    if res["error"] is None and rec["kind"] == "segments":
        model.selection = res["selection"].copy()
    elif res["error"] is None and rec["kind"] == "remove_small_segments":
        model.remove(res["hit"])


def trivial(rec, res):
    """Does a surface step that succeeded say nothing?  (The rule of the host test's "not trivial" conditions.)"""
    kind = rec["kind"]
    if kind == "segments":
        n = len(res["hit"])
        return res["stats"][1] in (1, n) or int(res["hit"].sum()) in (0, n)
    if kind in ("register", "register_loop"):
        return res["stats"][0] == 0 or res["stats"][3] != 0
    return res["removed"] in (0, len(res["hit"]))


def outputs(rec, res):
    """What the record's call returns, by name, from the model's result: float64 values as their uint64 bits."""
    if rec["call"] == "rows":
        return rm.outputs(rec, res)
    kind = rec["kind"]
    if kind == "remove_small_segments":
        return {"removed": res["removed"]}
    out = {"stats": tuple(int(v) for v in res["stats"])}
    if kind == "segments":
        out["selection"] = select_ref.words(res["selection"])
        if rec["labels"] is not None:
            out["labels"] = res["labels"]
        if not rec["stats"]:
            del out["stats"]
    elif kind == "register":
        out.update(moments=rr.bits64(res["moments"]).reshape(-1), step=rr.bits64(res["step"]).reshape(-1))
        out = {k: v for k, v in out.items() if k in rec["ask"]}
    else:
        out.update(pose=rr.bits64(res["pose"]).reshape(-1), rms=rr.bits64(np.array(res["rms"], f64)).reshape(-1))
    return out


def mismatches(got, want):
    """The names under which two dicts of `outputs` differ: arrays by dtype, shape and value (every float is there as
    its bit pattern), everything else by value.  No tolerance anywhere.  The one comparison of the GPU file; the host
    file hands it altered references."""
    if "_mean" in want:  # (a rows step: its own rule)
        return rm.mismatches(got, want)
    bad = sorted(set(got) ^ set(want))
    for k in sorted(set(got) & set(want)):
        x, y = got[k], want[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
                bad.append(k)
        elif x != y:
            bad.append(k)
    return sorted(bad)


class _Gen(rm._Gen):
    """rows_model._Gen's records, radii and edits under an agenda of directed chains of its own, with an rng chain of
    its own.  Thirty steps do not hold every chain of the issue in every sequence: the three long ones (HEAVY) stand in
    one sequence of a family each, by (seed + family) % 3, with the shorter ones beside them (README)."""

    def __init__(self, seed, family):
        super().__init__(seed, family)
        self.model = Model(family)
        fam = self.fam
        self.srng = np.random.default_rng([seed, fam, 6])  # (the surface steps' own chain)
        self.seg_k = 3 * seed + fam
        self.reg_k = 2 * seed + fam
        self.given_k = 3 * seed + fam
        self.kind_s = seed + fam
        self.seedless_done = False
        self.small_at = None
        mine = [e for j, e in enumerate(SHARED) if j % 3 == (seed + fam) % 3]
        move = [e for e in mine if e.startswith("move_")]
        rest = [e for e in mine if not e.startswith("move_")]
        heavy = HEAVY[(seed + fam) % 3]
        self.heavy = heavy
        self.last_edge = rest[1]
        # thirty steps: the third of SHARED with the removal of every point (four steps) stands beside the pipeline, the
        # one whose move the seeded chain holds beside the sort, the shortest beside the ties and the span step of the
        # removal; the last-chunk and the degenerate steps go where the family leaves room (README)
        sorts = em.allows_reorder(family)
        agenda = [("edge", rest[0])]
        if heavy == "ties":
            agenda += [("ties",), ("span", "segments", "beyond_span"), ("edge", move[0]), ("edge", rest[1])]
        elif heavy == "pipeline":
            agenda += [("pipeline",), ("span", "segments", "beyond_span"), ("edge", move[0]), ("icp",)]
            agenda += ([("last_chunk",), ("degenerate",)] if sorts else []) + [("edge", rest[1])]
        else:
            agenda += [("seeded", move[0]), ("span", "segments", "beyond_span"), ("edge", rest[1])]
            agenda += [("sorted",)] if sorts else [("last_chunk",), ("degenerate",)]
        agenda += [("span", "segments", "at_span"), ("span", "register", "pose_span")]
        if heavy == "ties":
            agenda.append(("span", "remove_small_segments", "beyond_span"))
        if heavy != "pipeline":  # (the removal of the small segments as an edit of its own, both calls behind it)
            agenda.append(("small",))
        self.agenda = agenda

    # -- the records of the new steps
    def _surface_radius(self, rank):
        """A radius that reaches the rank-th neighbour of some point: redrawn while a finite point is beyond the span of
        so small a radius or while it holds about more pairs than MAX_PAIRS (rows_model's rule)."""
        mo, radius = self.model, None
        for t in range(8):
            rq = self._radius(64, rank=rank)
            if rq is None:
                return None
            radius = rq[0]
            if not beyond_span(mo.xyz, radius).any() and self._pairs(radius) <= MAX_PAIRS:
                break
        return radius

    def _segments_step(self, edge=None, source=None, op=None, outside=None, seeded=None, oriented=None, limit=None, held=False,
                       radius=None, k=None, labels=False, where=None):
        """The record of a segments step on the current state, or None where the cloud allows none."""
        mo = self.model
        if mo.n == 0:
            return None
        self.seg_k += 1
        c = self.seg_k
        if source is None:  # (constant normals, which make the call section 6h's clustering, once in seven)
            source = "constant" if c % 7 == 0 else SOURCES[c % 2]
        if edge in ("beyond_span", "at_span"):
            radius = self._span_radius(mo.xyz, edge)
        elif radius is None:
            # (a radius that joins a block into ONE segment says nothing: the rank follows what the normals cut apart)
            rank = {"indexed": 6, "estimated": 8, "constant": 1 if mo.n < 1024 else 2}[source]
            radius = self._surface_radius(rank)
        if radius is None:
            return None
        if op is None:
            op, outside = em.OPS[c % len(em.OPS)], c % 3 == 0
        if seeded is None:  # (without a selection a seeded step hits nothing: one random step of a sequence; with one, every other)
            if mo.selection is not None and mo.selection.any():
                seeded = c % 2 == 0
            else:
                seeded = edge is None and not self.seedless_done
        self.seedless_done |= seeded and mo.selection is None
        if oriented is None:
            oriented = c % 4 == 1
        if limit is None:
            limit = source != "constant" and c % 2 == 0
        rec = {"call": "surface", "kind": "segments", "radius": float(radius), "source": source, "held": bool(held),
               "where": where or ("host", "device")[(c // 2) % 2], "k": int(k or 8), "nradius": float(radius),
               "cos_angle": float(f32({"indexed": 0.9, "estimated": 0.8, "constant": 0.99}[source])), "max_curvature": None,
               "min_points": 1, "max_points": 0, "oriented": bool(oriented), "seeded": bool(seeded), "op": op, "outside": bool(outside),
               "labels": PLACES[(c // 3) % 3] if labels is False else labels, "stats": c % 6 != 5, "edge": edge}
        if beyond_span(mo.xyz, radius).any():
            rec["state"] = self._qstate()
            return rec
        nrm, curv = mo.inputs(rec)
        if limit and source == "indexed":
            rec["max_curvature"] = float(f32(0.03))
        elif limit and source == "estimated":
            fin = curv[np.isfinite(curv)]
            rec["max_curvature"] = float(np.sort(fin)[3 * fin.size // 4]) if fin.size else float("inf")
        # the window: from the sizes of the segments themselves, so that about two thirds of the points hit, never all (a plain value of
        # the record; the labels are cached and serve the step itself)
        lim = rec["max_curvature"]
        lab = mo.labels(radius, rec["cos_angle"], nrm, None if lim is None else curv, np.inf if lim is None else lim, rec["oriented"])
        size = np.sort(np.bincount(lab)[lab])
        rec["min_points"] = int(max(2 if size[-1] >= 2 else 1, size[size.size // 3]))
        if c % 2 and size[-1] > rec["min_points"]:
            rec["max_points"] = int(size[-1] - 1)
        rec["state"] = self._qstate()
        return rec

    def _spacing(self, idx):
        """The median distance from (at most 48 of) the points idx to their nearest other finite point at another place."""
        mo = self.model
        p = mo.xyz[self._finite()].astype(f64)
        q = mo.xyz[idx[:: max(1, idx.size // 48)][:48]].astype(f64)
        d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        near = np.sqrt(np.where(d2 > 0, d2, np.inf).min(axis=1))
        near = near[np.isfinite(near)]
        return float(np.median(near)) if near.size else None

    def _part(self):
        """({"lo", "hi"}, its longest side): the box of the third of the finite points (64 .. 1024 of them) nearest to a point next to the last edit.
        Given points spread over parts that edits have thrown 10^4 apart or scaled by 1000 lie almost on a line, and no
        float64 path settles such a fit to README_register.md's bounds (the first draft did that, measured: 3e-9 rad
        against numpy's Kabsch); the edits' own book-keeping does not tell the parts apart, since a copy of a thrown
        point is a new point."""
        fin = self._finite()
        p = self.model.xyz[fin].astype(f64)
        d2 = ((p - self.model.xyz[int(self._near_hot(1)[0])].astype(f64)) ** 2).sum(axis=1)
        q = p[np.argsort(d2, kind="stable")[:min(1024, max(64, fin.size // 3))]]
        lo, hi = q.min(axis=0), q.max(axis=0)
        return {"lo": [float(v) for v in lo], "hi": [float(v) for v in hi]}, float((hi - lo).max())

    def _count(self):
        self.given_k += 1
        return GIVEN_ROTATION[self.given_k % len(GIVEN_ROTATION)]

    def _register_step(self, edge=None, kind="register", plane=None, source=None, count=None, part="all", posed=None, moved=True,
                       held=False, k=None, radius=None, far=False, iterations=6, where=None):
        """The record of a register step on the current state, or None where the cloud allows none."""
        mo = self.model
        if mo.n == 0 or self._finite().size == 0:
            return None
        self.reg_k += 1
        c = self.reg_k
        plane = bool(c % 2) if plane is None else plane
        posed = c % 4 < 3 if posed is None else posed
        count = self._count() if count is None else count
        if part == "all":
            part, side = self._part()
            # (point-to-plane's 6x6 system mixes lengths with pure numbers: on a part a thousand times larger or smaller
            # than the unit its condition alone, 10^7, is beyond the bounds; such a part is registered point to point)
            if plane and source != "constant" and not held and not 0.25 <= side <= 64.0:
                plane = False
        g = {"seed": int(self.srng.integers(1 << 30)), "count": int(count), "part": part, "motion": None,
             "specials": int(self.srng.integers(1, 3)) if self.special and count >= 63 and (edge is None or edge.startswith("behind")) else 0}
        idx = chosen(dict(g, count=max(count, 64)), mo)
        if idx.size == 0:
            return None
        s = self._spacing(np.unique(idx))
        if s is None or not am._ok_radius(4.0 * s):
            return None
        pose = None
        if far:  # (a shift that carries every given point out of the cloud's box by more than the radius)
            p = mo.xyz[self._finite()].astype(f64)
            M = np.eye(4)
            M[:3, 3] = -((p.max(axis=0) - p.min(axis=0)) + 64.0 * s)
            g["motion"] = [float(v) for v in M.reshape(-1)]
        elif moved:
            q = mo.xyz[idx].astype(f64)
            centre = q.mean(axis=0)
            extent = float(np.sqrt(((q - centre) ** 2).sum(axis=1).max()))
            g["motion"] = [float(v) for v in motion(centre, s, extent).reshape(-1)]
            if posed:  # (a perturbation of the motion: a little less of the angle, a little more of the shift)
                pose = [float(v) for v in motion(centre, s, extent, 0.85, 1.5)[:3].reshape(-1)]
        rec = {"call": "surface", "kind": kind, "radius": float(f32(4.0 * s)) if radius is None else float(radius), "plane": plane,
               "pose": pose, "given": g, "rows": ("host", "device")[(c // 2) % 2], "width": (3, 4)[(c // 4) % 2],
               "source": (source or SOURCES[(c // 2) % 2]) if plane else None, "held": bool(held),
               "where": where or ("host", "device")[(c // 3) % 2], "k": int(k or 8), "edge": edge}
        rec["nradius"] = rec["radius"]
        if kind == "register_loop":
            rec["iterations"] = int(iterations)
        else:
            rec["ask"] = list(ASKS[(c // 2) % 4] if edge is None or edge.startswith("behind") else ASKS[0])
        rec["state"] = self._qstate()
        return rec

    def _remove_small_step(self, edge=None, k=8, radius=None, min_points=None, limit=None, angle=None):
        mo = self.model
        if mo.n == 0:
            return None
        if edge == "beyond_span":
            radius = self._span_radius(mo.xyz, edge)
        elif radius is None:
            radius = self._surface_radius(8)
        if radius is None:
            return None
        rec = {"call": "surface", "kind": "remove_small_segments", "radius": float(radius), "k": int(k),
               "angle": float(math.acos(0.8)) if angle is None else angle, "max_curvature": float("inf") if limit is None else limit,
               "min_points": 2 if min_points is None else int(min_points), "edge": edge}
        if min_points is None and not beyond_span(mo.xyz, radius).any():
            e = mo.normals(k, radius)
            curv = e["curvature"][np.isfinite(e["curvature"])]
            if limit is None and curv.size:
                rec["max_curvature"] = float(np.sort(curv)[3 * curv.size // 4])
            lab = mo.labels(radius, f32(math.cos(rec["angle"])), e["normals"], e["curvature"], rec["max_curvature"], False)
            size = np.sort(np.bincount(lab)[lab])
            rec["min_points"] = int(max(2, min(5, size[size.size // 4])))  # (the smallest segments go)
        rec["state"] = self._qstate()
        return rec

    def _normals_step(self, edge, k, radius):
        rec = self._rows_step("normals", edge, k, radius)
        if rec is not None:
            rec["place"] = {"normals": "device", "curvature": "device", "found": None}
            rec["viewpoint"] = None
        return rec

    # -- the chains
    def _follower(self):
        """BOTH calls behind the edit: which comes first alternates along SHARED and from family to family; neither
        changes the cloud, so the second runs on what the edit left as well.  register alternates between its modes."""
        if self.override is not None:
            what, self.override = self.override, None
            return what()
        edge = "remove_all_then_append" if self.prev[1] == "append_empty" else self.prev[1]
        j = SHARED.index(edge) if edge in SHARED else len(self.recs)
        first = CALLS[(j + self.fam) % 2]
        # (behind the emptied cloud's append: 700 given points on 300, 37 or 255, so count > n and every point may win)
        count = 700 if edge == "remove_all_then_append" else None  # (None: the rotation's next)
        if count is None and edge == self.last_edge:  # (no given point and one given point, once in every family)
            count = {"ties": 0, "seeded": 1}.get(self.heavy)
        plane = (j + self.seed + self.fam) % 2 == 0
        # (an append or a removal has dropped the selection: the family's one step that is seeded without one)
        seedless = True if self.seed == SEEDS[self.fam % 3] and self.model.selection is None and not self.seedless_done else None
        if first == "segments":
            rec = self._segments_step("behind", seeded=seedless)
            if rec is not None:
                self._then(("register", "behind_second", plane, count))
            else:
                rec = self._register_step("behind", plane=plane, count=count)
            return rec
        rec = self._register_step("behind", plane=plane, count=count)
        self._then(("segments", "behind_second", None, None, None, seedless))
        return rec if rec is not None else self._continue(self.queue.pop(0))

    def _start(self, item):
        mo, what = self.model, item[0]
        big = mo.n > 3 * em.CHUNK
        if what == "edge":
            return nm._Gen._start(self, item)  # (its follower is the ("query", ...) item: _continue)
        if what == "span":
            if mo.n <= em.CHUNK:
                return None
            if item[1] == "segments":
                return self._segments_step(item[2], source="indexed" if item[2] == "beyond_span" else SOURCES[self.seed % 2],
                                           seeded=False)
            if item[1] == "remove_small_segments":
                return self._remove_small_step(item[2])
            return self._pose_span()
        if what == "ties":
            rec = self._copies("append_copies") if big else None
            if rec is not None:
                self._then(("mirrors", rec, mo.n), ("ties_register", rec, mo.n), ("ties_segments",), ("remove_originals", rec, mo.n),
                           ("same", "register", "ties_copies"), ("same", "segments", "ties_copies"), ("remove_copies", rec, mo.n),
                           ("same", "register", "ties_mirrors", {"plane": False, "source": None}), ("same", "segments", "ties_mirrors"))
            return rec
        if what == "pipeline":
            if not big:
                return None
            r = self._surface_radius(8)
            if r is None:
                return None
            rec = self._normals_step("pipeline", 8, r)
            if rec is not None:
                self._then(("pipeline_segments", r), ("pipeline_remove", r), ("pipeline_normals", r), ("pipeline_again",),
                           ("pipeline_register", r))
            return rec
        if what == "icp":
            rec = self._register_step("icp", "register_loop", plane=self.seed % 2 == 0, source="indexed", count=700, posed=True) if big else None
            if rec is not None:
                self._then(("icp_move",), ("same", "register_loop", "icp_again", None, True))
            return rec
        if what == "sorted":
            if not big:
                return None
            if not mo.sorted:
                self._then(("sorted",))
                return {"call": "reorder", "edge": None}
            rec = self._copies("append_copies_sorted")
            if rec is not None:
                self._then(("segments", "sorted", "indexed"), ("register", "sorted", True, 700, "indexed"), ("reorder",),
                           ("same", "segments", "reordered"), ("same", "register", "reordered"))
            return rec
        if what == "seeded":
            if not big:
                return None
            self._then(("seeded_segments",), ("register", "seeded", None, None), ("seeded_move", item[1]))
            return dict(self._random_select(), edge="selection")
        if what == "last_chunk":
            if not big:
                return None
            if mo.n % em.CHUNK < 8:  # (a last chunk of 40 points or more first)
                self._then(item)
                return self._block("append", 40, "grow_last_chunk")
            self._then(("register", "first_chunk_only", False, 63, None, "first_chunk", False), ("no_pair",))
            return self._register_step("last_chunk_only", plane=True, source="indexed", count=63, part="last_chunk", moved=False)
        if what == "small":
            if not big or self.i > STEPS - 3:
                return None
            loop = ("loop", "cleaned", self.seed % 2 == 1)
            if not np.isfinite(mo.xyz).all():
                # (the removal takes every non-finite point with it: registerPoints meets them in front of it)
                rec = self._continue(("loop", "before_small", self.seed % 2 == 1))
                if rec is not None:
                    self._then(("small_remove",), ("segments", "cleaned"))
                    return rec
            rec = self._remove_small_step("small")
            if rec is not None:
                self._then(*((("segments", "cleaned"), loop) if (self.seed + self.fam) % 2 else (loop, ("segments", "cleaned"))))
            return rec
        if what == "degenerate":
            if not big:
                return None
            self._then(("register", "degenerate_point", False, 2, None, "all", False))
            return self._register_step("degenerate_plane", plane=True, source="constant", count=700)
        raise ValueError(item)

    def _pose_span(self):
        """A register step whose POSE carries a finite given point beyond the span while the point itself lies inside."""
        rec = self._register_step("pose_span", plane=False, count=64, posed=False)
        if rec is None:
            return None
        G = scan(rec, self.model)
        if beyond_span(G, rec["radius"]).any() or not np.isfinite(G).all(axis=1).any():
            return None
        T = np.eye(4)[:3]
        T[0, 3] = 1.5 * 2.0 ** 20 * rec["radius"]
        rec["pose"] = [float(v) for v in T.reshape(-1)]
        return rec

    def _same(self, kind, edge, change=None, ref=False):
        """The last record of `kind` again on the state as it is now (the ties' given points are the very arrays of the
        first time: their originals are gone)."""
        j = max((i for i, r in enumerate(self.recs) if r["call"] == "surface" and r["kind"] == kind), default=None)
        if j is None or self.model.n == 0:
            return None
        rec = dict(self.recs[j], edge=edge, state=self._qstate())
        if kind != "segments" and (ref or edge.startswith("ties")):
            g = self.recs[j]["given"]
            rec["given"] = g if "ref" in g else {"ref": j}
        rec.update(change or {})
        return rec

    def _continue(self, item):
        mo, what = self.model, item[0]
        if what == "query":
            return self._follower()
        if what == "segments":
            return self._segments_step(item[1], *item[2:])
        if what == "register":
            plane, count = (item[2], item[3]) if len(item) > 3 else (None, None)
            source = item[4] if len(item) > 4 else None
            part = item[5] if len(item) > 5 else "all"
            moved = item[6] if len(item) > 6 else True
            return self._register_step(item[1], plane=plane, count=count, source=source, part=part, moved=moved)
        if what == "small_remove":
            return self._remove_small_step("small")
        if what == "loop":
            return self._register_step(item[1], "register_loop", plane=item[2], count=700, posed=True, iterations=4)
        if what == "same":
            return self._same(*item[1:])
        if what == "mirrors":
            return self._mirrors(item[1], item[2])
        if what == "ties_register":
            # (the originals themselves as given points, pose None: each finds itself at d2 = +0 ahead of its copies)
            if self.recs[-1]["call"] != "append_mirrors":
                return None
            src = nm.copied(item[1], mo.xyz[:item[2]])[:self.recs[-1]["mirrored"]]
            lo, hi = int(src.min()), int(src.max()) + 1
            rec = self._register_step("ties_originals", plane=True, source="indexed", count=0, posed=False, moved=False, where="host",
                                      radius=2.0 * self.recs[-1]["shift"])
            if rec is None:
                return None
            rec["given"] = {"indices": [int(v) for v in src], "seed": 0, "count": int(src.size), "part": [lo, hi], "motion": None, "specials": 0}
            return rec
        if what == "ties_segments":
            # (2.1 shifts: an original, its copies and its six mirrors are one pile within the radius, cut apart by the
            # normals their indices give them)
            if self.recs[-2]["call"] != "append_mirrors":
                return None
            return self._segments_step("ties_originals", "indexed", "replace", False, False, None, False, False,
                                       float(f32(2.1 * self.recs[-2]["shift"])), None, "host")
        if what == "remove_copies":
            # (behind the originals' removal the copies stand where the count of the removed points has shifted them)
            src, base = item[1], item[2]
            a = base - src["count"]
            return self._remove(("drop_range", a, a + src["count"] + src["count"] // 3), "remove_copies")
        if what == "pipeline_segments":
            rec = self._segments_step("pipeline", "estimated", "replace", False, False, False, True, True, item[1], 8, "device", "device")
            if rec is not None:
                rec["max_points"] = 0  # (the facade's removal has no upper bound)
            return rec
        if what == "pipeline_remove":
            seg = self.recs[-1]
            if seg["call"] != "surface" or self.results[-1]["error"] is not None:
                return None
            # (the facade takes an angle: the one whose cosine, through the host's libm, is the segments step's)
            angle = float(math.acos(0.8))
            if float(f32(math.cos(angle))) != seg["cos_angle"]:
                return None
            return self._remove_small_step("pipeline", 8, item[1], seg["min_points"], seg["max_curvature"], angle)
        if what == "pipeline_normals":
            return self._normals_step("pipeline_survivors", 8, item[1])
        if what == "pipeline_again":
            j = max((i for i, r in enumerate(self.recs) if r.get("kind") == "segments" and r["edge"] == "pipeline"), default=None)
            return None if j is None else dict(self.recs[j], edge="pipeline_survivors", state=self._qstate())
        if what == "pipeline_register":
            return self._register_step("pipeline", plane=True, source="estimated", count=700, held=True, k=8, radius=item[1], where="device")
        if what == "seeded_segments":
            op, outside, oriented = SEEDED[self.fam]
            return self._segments_step("seeded", None, op, outside, True, oriented)
        if what == "seeded_move":
            def again():
                self._then(("register", "behind_second", None, 64))
                return self._same("segments", "seeded_again")
            self.override = again
            rec = nm._Gen._start(self, ("edge", item[1]))
            if rec is None:
                self.override = None
            return rec
        if what in ("remove_originals", "reorder", "append_empty", "icp_move", "sorted"):
            return nm._Gen._continue(self, item) if what != "sorted" else self._start(item)
        if what == "no_pair":
            return self._register_step("no_pair", plane=False, count=64, posed=False, far=True)
        return self._start(item)

    def _random(self):
        mo = self.model
        if mo.n > 0 and self.srng.random() < 0.5:
            self.kind_s += 1
            rec = self._segments_step() if self.kind_s % 2 else self._register_step()
            if rec is not None:
                return rec
        return wm._Gen._random(self)

    # -- what the last edit touched
    def _note(self, rec, args, before):
        if rec["call"] != "surface":
            return rm._Gen._note(self, rec, args, before)
        res = self.results[-1]
        if rec["kind"] == "remove_small_segments" and res["error"] is None:
            nm._Gen._note(self, dict(rec, call="remove_originals"), {"bits": res["hit"]}, before)
        elif rec["kind"] == "segments" and res["error"] is None:
            self.selection_by = "segments"
        self.prev, self.follow = (rec["kind"], rec["edge"]), False

    def _track(self, rec, args, n0):
        if rec["call"] != "surface":
            return rm._Gen._track(self, rec, args, n0)
        res = self.results[-1]
        if rec["kind"] == "remove_small_segments" and res["error"] is None:
            if not res["hit"].any():
                self.level, self.thrown = np.zeros(0, np.int8), np.zeros(0, bool)
            else:
                self.level, self.thrown = self.level[res["hit"]], self.thrown[res["hit"]]

    def step(self, i):
        """A chain in progress goes on; else upkeep (a start cloud of three chunks or fewer is asked once, then grows);
        else the next chain of the agenda starts; else a random step, half of them segments and register in turn."""
        rec, mo, self.i = None, self.model, i
        if i == 0:
            rec = self._block("upload", int(self.rng.choice(em.START_COUNTS)))
        while rec is None and self.queue:
            rec = self._continue(self.queue.pop(0))
        if rec is None and 0 < mo.n <= 3 * em.CHUNK and self.prev[0] == "upload" and self.heavy != "pipeline":
            rec = self._segments_step("small") if (self.seed + self.fam) % 2 else self._register_step("small", count=63)
        if rec is None and mo.n <= 3 * em.CHUNK:
            rec = self._block("append", int(self.arng.integers(3 * em.CHUNK + 1, 3000)))
        if rec is None and self.agenda:
            for a in list(self.agenda):
                rec = self._start(a)
                if rec is not None:
                    self.agenda.remove(a)
                    break
        if rec is None:
            rec = self._random()
        before = mo.copy()
        args, n0 = materialize(rec, mo, self.past), mo.n
        res = apply(mo, rec, args)
        self.results.append(res)
        self._track(rec, args, n0)
        self._note(rec, args, before)
        assert mo.n <= em.N_MAX and self.level.shape == self.thrown.shape == (mo.n,)
        self.past.append(args)
        self.recs.append(rec)
        self.done = (rec, args, res, n0, before.selection, None if mo.selection is None else mo.selection.copy())
        return rec


def replay(seed, family, steps=STEPS):
    """[(record, arguments, result, n before, selection before, selection after)] of the sequence on the model alone, a
    pure function of the arguments (result: None for a step that is neither a surface nor a rows step).  The references
    are computed once, while the sequence is drawn, and shared by every test that needs them: cached, read, never
    changed."""
    return _replay(int(seed), family, int(steps))


@functools.lru_cache(maxsize=None)
def _replay(seed, family, steps):
    g, out = _Gen(seed, family), []
    for i in range(steps):
        g.step(i)
        out.append(g.done)
    return tuple(out)


def sequence(seed, family, steps=STEPS):
    """`steps` step records: write_model.sequence's calls with surface steps and their directed edits among them."""
    return tuple(r[0] for r in replay(seed, family, steps))


def frame_steps(steps):
    return em.frame_steps(steps)


# Regressions: prefixes of random sequences that failed on the library, as literal steps: {name: (family, [records])}.
REGRESSIONS = {}
