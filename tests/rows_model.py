"""nearest_model.py with the two per-point row calls in it (include/rtr_statistics.h section 6n, include/rtr_normals.h
section 6o): `Model` gains `statistical`, `normals` and `cleanup` (ProjectCloud.removeStatisticalOutliers), the sequences
gain their steps among the appends, removals, moves, masks, selections, sorts and writes write_model draws -- so that
rtr_select_statistical and rtr_estimate_normals, which RETURN a value per resident point in upload order, run on clouds
that edits have rewritten in place and whose indices removals have renumbered.  test_gpu_rows_sequences.py drives the
library with them, test_rows_model_host.py checks this file without a GPU.  numpy only.

Results come from the brute-force rows alone (normals_ref.rows_brute: section 6n's row is section 6o's without the
indices, so one set of rows serves both calls of a step pair), then statistical_ref.select, normals_ref.estimate and
select_ref.combine; analysis_model.beyond_span predicts RTR_ERR_UNSUPPORTED.

Records.  "call" = "rows"; "kind": "statistical", "normals" or "cleanup"; "k"; "radius"; statistical: "std_mul",
"threshold" (None, or the float t an earlier step of the sequence returned in the model: RTR_STAT_THRESHOLD_GIVEN), "op",
"outside"; normals: "viewpoint" (None or three floats); cleanup: "std_mul"; "place": where each output array is asked for
("host", "device" or None: absent), by name; "edge": None, "beyond_span", "at_span" or the name of the directed step;
"state": nearest_model's.  "append_near": appends ONE point within 0.05 radius per axis of resident point "at".  "append_mirrors": see `mirrors`; a
"remove_originals" record of the same "seed" and "count" removes the points they were made from.  Every other record is
nearest_model's."""
import functools

import numpy as np

import analysis_model as am
import edit_model as em
import nearest_model as nm
import normals_ref as nf
import select_ref
import statistical_ref as sf
import write_model as wm
from analysis_model import FAMILIES, axis_in_span, beyond_span, pose_for  # noqa: F401

f32 = np.float32
SEEDS = (1, 2, 3)
STEPS = 30
KINDS = ("statistical", "normals", "cleanup")
CALLS = ("statistical", "normals")
KS = (1, 2, 7, 8, 9, 16, 17, 33, 64)  # (every capacity bucket of both kernels)
COPY_KS = (2, 3, 8)
STD_MULS = (0.0, 0.5, 1.0, 2.0, -0.5)
PLACES = ("host", "device", None)
COMBINING = ("add", "subtract", "intersect", "toggle")
SPAN_STEPS = (("statistical", "beyond_span"), ("normals", "at_span"), ("normals", "beyond_span"), ("statistical", "at_span"))
SHARED = nm.SHARED
EMPTY_APPEND = nm.EMPTY_APPEND
HEAVY = ("copies", "sorted", "selected", "same_n")  # (a sequence of a family that sorts leaves one of the last three out)
MAX_PAIRS = 600_000  # (a drawn radius is redrawn while about more pairs than these lie within it)
ARRAYS = {"statistical": ("mean", "found"), "normals": ("normals", "curvature", "found")}


# ---- the rows, computed once per (cloud, radius) ------------------------------------------------------------------------
_ROWS = {}


def rows_of(xyz, radius, k):
    """normals_ref.rows_brute(xyz, radius, K) of some K >= k: shared by the steps that ask one cloud for one radius."""
    key = (hash(xyz.tobytes()), xyz.shape[0], float(radius))
    hit = _ROWS.get(key)
    if hit is None or hit[0] < k:
        if len(_ROWS) >= 4:
            _ROWS.pop(next(iter(_ROWS)))
        hit = _ROWS[key] = (k, nf.rows_brute(xyz, radius, k))
    return hit[1]


# ---- the model ----------------------------------------------------------------------------------------------------------
class Model(nm.Model):
    """nearest_model.Model with the two calls and the clean-up.  Each returns a dict: "error" (None or "unsupported":
    the facade raises RtrError with RTR_ERR_UNSUPPORTED and nothing changes) and the call's outputs."""

    def copy(self):
        m = Model(self.family)
        m.__dict__.update(em.Model.copy(self).__dict__)
        return m

    def statistical(self, k, radius, std_mul=1.0, threshold=None, op="replace", outside=False):
        assert self.n > 0
        if beyond_span(self.xyz, radius).any():
            return {"error": "unsupported"}
        _, d2, found = nf.cut(rows_of(self.xyz, radius, k), k)
        s = sf.select(self.xyz, radius, k, std_mul, threshold, rows_found=(d2, found))
        count = self._combine(op, outside, s["hit"])
        return {"error": None, "hit": s["hit"], "mean": s["mean"], "found": s["found"], "moments": s["moments"],
                "stats": (count,) + s["stats"], "given": threshold is not None, "selection": self.selection.copy()}

    def normals(self, k, radius, viewpoint=None):
        """Reads and changes nothing of the model."""
        assert self.n > 0
        if beyond_span(self.xyz, radius).any():
            return {"error": "unsupported"}
        e = nf.estimate(self.xyz, radius, k, viewpoint, rows_k=rows_of(self.xyz, radius, k))
        return {"error": None, "normals": e["normals"], "curvature": e["curvature"], "found": e["found"], "stats": e["stats"],
                "index": e["index"], "d2": e["d2"], "C": e["C"]}

    def cleanup(self, k, radius, std_mul=1.0):
        """ProjectCloud.removeStatisticalOutliers: the points that are no hit go (non-finite and isolated ones among
        them), the survivors are renumbered in order, the selection is dropped as any removal drops it."""
        assert self.n > 0
        if beyond_span(self.xyz, radius).any():
            return {"error": "unsupported"}
        hit = self.copy().statistical(k, radius, std_mul)["hit"]
        self.remove(hit)
        return {"error": None, "hit": hit, "removed": int((~hit).sum())}


# ---- step records ---------------------------------------------------------------------------------------------------------
def eye_of(P):
    """The eye position of an edit_model.pose_for camera."""
    P = np.asarray(P, np.float64).reshape(4, 4)
    return -np.linalg.solve(P[:3, :3], P[:3, 3])


def near_point(rec, model):
    rng = np.random.default_rng(rec["data"])
    with np.errstate(all="ignore"):
        x = model.xyz[rec["at"]].astype(np.float64) + rng.uniform(-0.05, 0.05, 3) * rec["radius"]
    return np.ascontiguousarray(x.astype(f32).reshape(1, 3)), rng.integers(0, 256, size=(1, 3)).astype(np.uint8)


def mirrors(rec, xyz):
    """(float32 (6 mirrored, 3), the originals' indices): the six points one "shift" (a power of two) beside each of the
    first "mirrored" of the "count" finite points the seed chooses (an append_copies record's, among the first "base"), along +x, -x, +y, -y, +z, -z.  Where the sums are exact in float32 -- nearly
    everywhere: the shift is a multiple of the coordinates' last place -- an original has six neighbours at one d2 and
    each of the six has four at another: ties between points that do NOT coincide, which the index alone orders."""
    src = nm.copied(rec, xyz)[:rec["mirrored"]]
    out = np.repeat(xyz[src], 6, axis=0)
    with np.errstate(all="ignore"):
        for a in range(3):
            out[2 * a::6, a] += f32(rec["shift"])
            out[2 * a + 1::6, a] -= f32(rec["shift"])
    return np.ascontiguousarray(out), src


def materialize(rec, model, past=None):
    call = rec["call"]
    if call == "append_mirrors":
        xyz, src = mirrors(rec, model.xyz[:rec["base"]])
        rgb = np.random.default_rng(rec["seed"] + 1).integers(0, 256, size=(xyz.shape[0], 3)).astype(np.uint8)
        return {"xyz": xyz, "rgb": rgb, "src": np.repeat(src, 6)}
    if call == "rows":
        vp = rec.get("viewpoint")
        return {"viewpoint": None if vp is None else np.array(vp, f32)}
    if call == "append_near":
        xyz, rgb = near_point(rec, model)
        return {"xyz": xyz, "rgb": rgb}
    return nm.materialize(rec, model, past)


def apply(model, rec, args):
    """-> the result of a rows step, None for every other call."""
    call = rec["call"]
    if call == "rows":
        if rec["kind"] == "statistical":
            return model.statistical(rec["k"], rec["radius"], rec["std_mul"], rec["threshold"], rec["op"], rec["outside"])
        if rec["kind"] == "normals":
            return model.normals(rec["k"], rec["radius"], args["viewpoint"])
        return model.cleanup(rec["k"], rec["radius"], rec["std_mul"])
    if call in ("append_near", "append_mirrors"):
        return model.append(args["xyz"], args["rgb"])
    return nm.apply(model, rec, args)


def advance(model, rec, res):
    """What a rows step does to the model, from the result `apply` gave on a copy: nothing is computed again."""
    if res["error"] is None and rec["kind"] == "statistical":
        model.selection = res["selection"].copy()
    elif res["error"] is None and rec["kind"] == "cleanup":
        model.remove(res["hit"])


def trivial(rec, res):
    """Does a rows step that succeeded say nothing?  (The rule of the host test's "not trivial" conditions.)"""
    if rec["kind"] == "statistical":
        return int(res["hit"].sum()) in (0, len(res["hit"])) or not res["found"].any()
    if rec["kind"] == "normals":
        return res["stats"][0] == 0
    return res["removed"] in (0, len(res["hit"]))


def outputs(rec, res):
    """What the record's call returns, by name, from the model's result: the arrays that were asked for, the stats, the
    moments and the selection's words.  The names that start with "_" are no outputs: what `mismatches` needs to hold
    the moments to statistical_ref.moments_tolerance and the hits to the t that was returned."""
    kind = rec["kind"]
    if kind == "cleanup":
        return {"removed": res["removed"]}
    out = {"stats": tuple(int(v) for v in res["stats"])}
    for name in ARRAYS[kind]:
        if rec["place"][name] is not None:
            out[name] = res[name]
    if kind == "statistical":
        out.update(moments=tuple(float(v) for v in res["moments"]), selection=select_ref.words(res["selection"]),
                   _mean=res["mean"], _found=res["found"], _hit=res["hit"], _given=res["given"])
    return out


def _same_array(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))


def mismatches(got, want):
    """The names under which two dicts of `outputs` differ: arrays by dtype, shape and bits, the stats by value.  The
    moments follow test_gpu_statistical.py's rule against numpy: each within statistical_ref.moments_tolerance(c)
    relative (a given threshold comes back as it went in), and the hits recomputed from the RETURNED t are exactly the
    reference's ("hit").  The one comparison of the GPU file; the host file hands it altered references."""
    a = {k for k in got if not k.startswith("_")}
    b = {k for k in want if not k.startswith("_")}
    bad = sorted(a ^ b)
    for k in sorted(a & b):
        x, y = got[k], want[k]
        if k == "moments":
            tol = sf.moments_tolerance(int((want["_found"] > 0).sum()))
            ok = len(x) == 3 and all(abs(g - w) <= tol * abs(w) for g, w in zip(x, y))  # (a NaN fails)
            if want["_given"]:
                ok = ok and x[2] == y[2]
            if not ok:
                bad.append(k)
            elif not np.array_equal(sf.hits(want["_mean"], want["_found"], x[2]), want["_hit"]):
                bad.append("hit")
        elif isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            if not _same_array(x, y):
                bad.append(k)
        elif x != y:
            bad.append(k)
    return sorted(bad)


class _Gen(nm._Gen):
    """analysis_model._Gen's parameter rules (through nearest_model._Gen, whose records of copies and whose chains of
    followed edits are reused) under an agenda of its own, with an rng chain of its own."""

    def __init__(self, seed, family):
        super().__init__(seed, family)
        self.model = Model(family)
        fam = self.fam = sorted(FAMILIES).index(family)
        self.rrng = np.random.default_rng([seed, fam, 5])  # (the rows steps' own chain)
        # the rotation of k: the first of KS -- the sequence's own third of it (by seed) in front, so that three seeds
        # hold all nine -- that the call has not run with success in this sequence; a clean-up, whose two followers run
        # both calls at its k, takes the first that either call still lacks of its third
        self.k_used = {kind: set() for kind in KINDS}
        self.kind_k = seed + fam
        self.op_k = 2 * seed + fam
        self.place_k = {"statistical": 4 * seed + fam, "normals": 10 * seed + 5 * fam}
        self.view_k = seed + fam
        self.mul_k = seed + 2 * fam
        self.eye_done = False
        self.results = []
        self.override = None  # what the next follower is, where a chain names it
        self.again_done = False  # a second clean-up has run among the random steps
        self.copy_at = None   # the step of the copy chain's first normals record
        # (a third of SHARED, which third by seed AND family: remove_all_then_append falls to another seed from family
        # to family, so that its appends of 300, 37 and 255 points, by seed, all occur)
        mine = [e for j, e in enumerate(SHARED) if j % 3 == (seed + fam) % 3]
        move = [e for e in mine if e.startswith("move_")]
        rest = [e for e in mine if not e.startswith("move_")]
        # (thirty steps hold the copies and ONE of the other three chains beside the rest: each in one sequence of a family)
        heavy = ["copies", HEAVY[1 + (seed + fam) % 3]]
        if not em.allows_reorder(family) and "sorted" in heavy:
            heavy.remove("sorted")
        spans = [("span",) + s for s in SPAN_STEPS[seed % 4:] + SPAN_STEPS[:seed % 4]]
        if seed == SEEDS[fam % 3]:
            spans.append(("span", "cleanup", "beyond_span"))
        at = fam // 2 % 2  # (the same-n chain stands behind one of the two, but not on the 37 points of an emptied cloud)
        at = 1 - at if rest[at] == "remove_all_then_append" else at
        agenda = [("same_n" if "same_n" in heavy and j == at else "edge", rest[j]) for j in range(2)]
        # (the clean-up behind the move and the sort: on a cloud with a chunk of mixed scales, sorted where the family sorts)
        agenda += [("copies",), spans[0]]
        agenda.append(("selected", move[0]) if "selected" in heavy else ("edge", move[0]))
        agenda += [spans[1]] + ([("sorted",)] if "sorted" in heavy else []) + [("cleanup",), spans[2]] + spans[3:]
        self.agenda = agenda

    # -- the records of the new steps
    def _place(self, kind, present=False):
        c = self.place_k[kind]
        self.place_k[kind] += 1
        names = ARRAYS[kind]
        if present:
            return {name: PLACES[(c + j) % 2] for j, name in enumerate(names)}
        return {name: PLACES[(c // 3 ** j) % 3] for j, name in enumerate(names)}

    def _std_mul(self):
        self.mul_k += 1  # (in rotation: fifteen draws did not always hold all five)
        return float(STD_MULS[self.mul_k % len(STD_MULS)])

    def _viewpoint(self):
        mo = self.model
        self.view_k += 1
        fin = mo.xyz[self._finite()].astype(np.float64)
        if self.view_k % 2 or not len(fin):
            return None
        if not self.eye_done and self.i >= 8:
            with np.errstate(all="ignore"):
                eye = eye_of(pose_for(mo, self.i)).astype(f32)
            if np.isfinite(eye).all():
                self.eye_done = True
                return [float(v) for v in eye]
        lo, hi = fin.min(axis=0), fin.max(axis=0)
        with np.errstate(all="ignore"):
            v = (lo - 0.5 * (hi - lo) + self.rrng.random(3) * 2.0 * (hi - lo)).astype(f32)
        return [float(x) for x in v] if np.isfinite(v).all() else None

    def _rows_step(self, kind, edge=None, k=None, radius=None, present=False, op=None, outside=None, threshold=None,
                   std_mul=None, pair=False):
        """The record of a rows step of `kind` on the current state, or None where the cloud allows none."""
        mo, fin = self.model, self._finite().size
        if mo.n == 0:
            return None
        span = edge in ("beyond_span", "at_span")
        if k is None:
            third = {c: [v for j, v in enumerate(KS) if (j + (c == "statistical")) % 3 == self.seed % 3] for c in CALLS}
            if kind == "cleanup" or pair:  # (both calls run at this k: what either still lacks of its third)
                order = [v for c in ("normals", "statistical") for v in third[c] if v not in self.k_used[c]]
                k = (order + [KS[(self.fam + len(self.recs)) % len(KS)]])[0]
            else:
                rest = [KS[(self.fam + j) % len(KS)] for j in range(len(KS))]
                order = third[kind] + [v for v in rest if v not in third[kind]]
                k = next((v for v in order if v not in self.k_used[kind]), order[0])
            if 0 < fin < 64:
                k = 64  # (more than there are points to find)
        if span:
            radius = self._span_radius(mo.xyz, edge)
            if radius is None:
                return None
        elif radius is None:
            # (redrawn while a finite point is beyond the span of so small a radius, or while so large a radius -- round a
            # q in a part an edit has scaled up -- holds a whole dense part: the reference lists every accepted pair)
            for t in range(8):
                rq = self._radius(64, rank=k)
                if rq is None:
                    return None
                radius = rq[0]
                if not beyond_span(mo.xyz, radius).any() and self._pairs(radius) <= MAX_PAIRS:
                    break
        rec = {"call": "rows", "kind": kind, "k": int(k), "radius": float(radius), "edge": edge}
        if kind == "statistical":
            if op is None:
                self.op_k += 1
                op, outside = em.OPS[self.op_k % len(em.OPS)], self.op_k % 3 == 0
            rec.update(std_mul=self._std_mul() if std_mul is None else std_mul,
                       threshold=threshold, op=op, outside=bool(outside), place=self._place(kind, present))
        elif kind == "normals":
            rec.update(viewpoint=self._viewpoint(), place=self._place(kind, present))
        else:
            rec.update(std_mul=self._std_mul() if std_mul is None else std_mul)
        if not beyond_span(mo.xyz, radius).any():  # (a k counts as run when the step succeeds, an at_span step too)
            for c in (CALLS if kind == "cleanup" else (kind,)):
                self.k_used[c].add(int(k))
        rec["state"] = self._qstate()
        return rec

    def _pairs(self, radius):
        """About how many pairs lie within the radius, from 48 finite points in float64: a measure to choose by."""
        fin = self._finite()
        p = self.model.xyz[fin].astype(np.float64)
        q = p[np.random.default_rng(fin.size).integers(fin.size, size=48)]
        with np.errstate(all="ignore"):
            near = (((q[:, None, :] - p[None, :, :]) ** 2).sum(axis=2) <= float(radius) ** 2).sum()
        return int(near) * fin.size // 48

    def _follower(self):
        if self.override is not None:
            what, self.override = self.override, None
            return what()
        # (BOTH calls behind the edit, on one set of rows: which comes first alternates along SHARED and from family
        # to family; rtr_estimate_normals changes nothing, so the second runs on the cloud the edit left as well)
        edge = "remove_all_then_append" if self.prev[1] == "append_empty" else self.prev[1]
        first = CALLS[(SHARED.index(edge) + self.fam) % 2] if edge in SHARED else "normals"
        rec = self._rows_step(first, pair=True)
        if rec is not None:
            self._then(("rows", CALLS[1 - CALLS.index(first)], "second", rec["k"], rec["radius"]))
        return rec

    def _copy_radius(self, src):
        """1.0001 x the distance from a copied point to its 4th DISTINCT neighbour (its copies lie at distance zero)."""
        mo = self.model
        p = mo.xyz[self._finite()].astype(np.float64)
        for j in src[:8]:
            d = np.unique(np.sqrt(((p - mo.xyz[j].astype(np.float64)) ** 2).sum(axis=1)))
            if d.size >= 5:
                with np.errstate(all="ignore"):
                    r = f32(1.0001 * d[4])
                if am._ok_radius(r) and not beyond_span(mo.xyz, r).any():
                    return float(r)
        return None

    def _mirrors(self, copies, base):
        """The record of an append_mirrors step beside the originals of an append_copies record (the same seed and
        count, chosen among the first `base` points): the shift is the power of two at or below a quarter of the
        originals' median distance to their nearest other point."""
        mo, fin = self.model, self._finite()
        count = min(copies["count"], 96)  # (the first 96 of the copied points at the most: six points each)
        if mo.n + 6 * count > em.N_MAX:
            return None
        rec = {"call": "append_mirrors", "seed": copies["seed"], "count": copies["count"], "mirrored": count, "base": int(base),
               "edge": "append_mirrors"}
        p = mo.xyz[fin].astype(np.float64)
        q = mo.xyz[nm.copied(rec, mo.xyz[:base])[:count]].astype(np.float64)
        d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        near = np.sqrt(np.median(np.where(d2 > 0, d2, np.inf).min(axis=1)))
        if not np.isfinite(near) or near <= 0:
            return None
        rec["shift"] = float(2.0 ** np.floor(np.log2(0.25 * near)))
        return rec if am._ok_radius(rec["shift"]) else None

    # -- the chains
    def _start(self, item):
        mo, what = self.model, item[0]
        big = mo.n > 3 * em.CHUNK
        if what == "edge":
            return nm._Gen._start(self, item)  # (its follower is the ("query", ...) item: _continue)
        if what == "span":
            if mo.n <= em.CHUNK:
                return None
            return self._rows_step(item[1], item[2])
        if what == "copies":
            # (exact copies tie with points of the same coordinates, which no output shows: the mirrors of the same
            # originals stand beside them, see `mirrors`)
            rec = self._copies("append_copies") if big else None
            if rec is not None:
                self._then(("mirrors", rec, mo.n), ("copy_normals",), ("remove_originals", rec, mo.n), ("again", None, "survivors"))
            return rec
        if what == "sorted":
            if not big:
                return None
            if not mo.sorted:
                self._then(("sorted",))
                return {"call": "reorder", "edge": None}
            rec = self._copies("append_copies_sorted")
            if rec is not None:
                self._then(("copy_normals",), ("reorder",), ("again", None, "reordered"))
            return rec
        if what == "selected":
            if not big:
                return None
            j = len(self.recs) + 1
            self._then(("selected_statistical",), ("rows", "normals", "selected"), ("selected_move", item[1], j))
            return dict(self._random_select(), edge="selection")
        if what == "cleanup":
            if not big or self.i > STEPS - 3:
                return None
            rec = self._rows_step("cleanup", "cleanup" if len(item) == 1 else "cleanup_again")
            if rec is not None:
                self._then(("rows", "normals", "cleaned", rec["k"], rec["radius"]), ("rows", "statistical", "cleaned", rec["k"], rec["radius"]))
            return rec
        if what == "same_n":
            # (behind the seed's second edit: its follower is the chain's first statistical step)
            j = [None]

            def first():
                rec = self._rows_step("normals", pair=True)
                if rec is not None:
                    self._then(("same_n_first", rec["k"], rec["radius"]))
                return rec
            self.override = first
            rec = nm._Gen._start(self, ("edge", item[1]))
            if rec is None:
                self.override = None
            return rec
        raise ValueError(item)

    def _continue(self, item):
        mo, what = self.model, item[0]
        if what == "query":
            return self._follower()
        if what == "rows":
            return self._rows_step(item[1], item[2], *item[3:])
        if what == "again":
            j = self.copy_at if item[1] is None else item[1]
            if j is None or self.results[j] is None:
                return None
            return dict(self.recs[j], edge=item[2], state=self._qstate())
        if what == "mirrors":
            return self._mirrors(item[1], item[2])
        if what == "copy_normals":
            self.copy_at = None
            src = self.past[-1]["src"]
            r = self._copy_radius(mo.n - src.size + np.arange(src.size // 4 * 3, src.size))  # (the copies of the triples first)
            if r is None:
                return None
            self.copy_at = len(self.recs)
            return self._rows_step("normals", "copies", COPY_KS[(self.seed + self.fam) % 3], r)
        if what == "same_n_first":
            rec = self._rows_step("statistical", "same_n", item[1], item[2], present=True, op="replace", outside=False)
            j = len(self.recs)
            if rec is not None:
                self._then(("append_near", j), ("again", j, "same_n_plus_1"), ("remove_last",), ("again", j, "same_n_again"))
            return rec
        if what == "selected_statistical":
            op = COMBINING[(self.seed + self.fam) % 4]
            return self._rows_step("statistical", "selected", op=op, outside=(self.seed + self.fam) % 2 == 0)
        if what == "selected_move":
            def given():
                first = self.results[item[2]]
                if first is None or first.get("error") is not None:
                    return self._rows_step("statistical", "given")
                src = self.recs[item[2]]
                self._then(("rows", "normals", "second", src["k"], src["radius"]))  # (both calls behind the move)
                return self._rows_step("statistical", "given", src["k"], src["radius"], op="replace", outside=False,
                                       threshold=float(first["moments"][2]), std_mul=1.0)
            self.override = given
            rec = nm._Gen._start(self, ("edge", item[1]))
            if rec is None:  # (no part of the cloud may move so: the given threshold on the cloud as it is)
                self.override = None
                return given()
            return rec
        if what == "append_near":
            src = self.recs[item[1]]
            at = int(self._near_hot(1)[0])
            if mo.n >= em.N_MAX:
                return None
            return {"call": "append_near", "at": at, "radius": src["radius"], "data": int(self.rrng.integers(1 << 30)),
                    "edge": "append_one"}
        if what == "remove_last":
            return self._remove(("drop_range", mo.n - 1, mo.n), "remove_last_point") if mo.n >= 2 else None
        if what in ("remove_originals", "reorder", "append_empty"):
            return nm._Gen._continue(self, item)
        return self._start(item)

    def _need(self):
        """The steps the agenda still needs, at the most."""
        cost = {"span": 1, "selected": 7, "copies": 5, "sorted": 6, "edge": 5, "cleanup": 3, "same_n": 9}
        return 1 + sum(cost[a[0]] for a in self.agenda)

    def _random(self):
        mo = self.model
        third = self.rrng.random() < 0.34
        # (the second clean-up takes the first random step that leaves the agenda its steps: there are few random steps)
        late = mo.n > 3 * em.CHUNK and not self.again_done and self.i >= 6 and STEPS - self.i - 3 >= self._need()
        if mo.n > 0 and (third or late):
            for j in range(len(KINDS)):
                kind = KINDS[(self.kind_k + 1 + j) % len(KINDS)] if not late or j else "cleanup"
                if kind == "cleanup" and not late:
                    continue
                rec = self._start(("cleanup", "again")) if kind == "cleanup" else self._rows_step(kind)
                if rec is not None:
                    self.again_done |= kind == "cleanup"
                    self.kind_k = KINDS.index(kind)
                    return rec
        return wm._Gen._random(self)

    # -- what the last edit touched
    def _note(self, rec, args, before):
        call = rec["call"]
        if call == "rows":
            res = self.results[-1]
            if rec["kind"] == "cleanup" and res["error"] is None:
                nm._Gen._note(self, dict(rec, call="remove_originals"), {"bits": res["hit"]}, before)
            elif rec["kind"] == "statistical" and res["error"] is None:
                self.selection_by = "statistical"
            self.prev, self.follow = (rec["kind"], rec["edge"]), False
            return
        if call in ("append_near", "append_mirrors"):
            nm._Gen._note(self, dict(rec, call="append_copies"), args, before)
        else:
            nm._Gen._note(self, rec, args, before)
        self.prev = (call, rec["edge"])

    def _track(self, rec, args, n0):
        call = rec["call"]
        if call == "rows":
            res = self.results[-1]
            if rec["kind"] == "cleanup" and res["error"] is None:
                self.level, self.thrown = self.level[res["hit"]], self.thrown[res["hit"]]
        elif call in ("append_near", "append_mirrors"):
            nm._Gen._track(self, dict(rec, call="append_copies"), args, n0)
        else:
            nm._Gen._track(self, rec, args, n0)

    def step(self, i):
        """A chain in progress goes on; else upkeep (a start cloud of three chunks or fewer is asked once, then grows);
        else the next chain of the agenda starts, at every other step or when the steps left are no more than the
        agenda needs; else a random step, a third of them statistical, normals and cleanup in rotation."""
        rec, mo, self.i = None, self.model, i
        if i == 0:
            rec = self._block("upload", int(self.rng.choice(em.START_COUNTS)))
        while rec is None and self.queue:
            rec = self._continue(self.queue.pop(0))
        if rec is None and 0 < mo.n <= 3 * em.CHUNK and self.prev[0] == "upload":
            rec = self._rows_step(CALLS[(self.seed + self.fam) % 2])
        if rec is None and mo.n <= 3 * em.CHUNK:
            rec = self._block("append", int(self.arng.integers(3 * em.CHUNK + 1, 3000)))
        if rec is None and self.agenda:
            if i % 2 == 0 or STEPS - i <= self._need():
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
    pure function of the arguments (result: None for a step that is no rows step).  The references are computed once,
    while the sequence is drawn, and shared by every test that needs them: cached, read, never changed."""
    return _replay(int(seed), family, int(steps))


@functools.lru_cache(maxsize=None)
def _replay(seed, family, steps):
    g, out = _Gen(seed, family), []
    for i in range(steps):
        g.step(i)
        out.append(g.done)
    return tuple(out)


def sequence(seed, family, steps=STEPS):
    """`steps` step records: write_model.sequence's calls with rows steps and their directed edits among them."""
    return tuple(r[0] for r in replay(seed, family, steps))


def frame_steps(steps):
    return em.frame_steps(steps)


# Regressions: prefixes of random sequences that failed on the library, as literal steps: {name: (family, [records])}.
REGRESSIONS = {}
