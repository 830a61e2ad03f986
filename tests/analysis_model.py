"""write_model.py with the analysis calls in it (include/rtr.h sections 6g - 6k): `Model` gains `voxel`, `neighbours`,
`clusters`, `near`, `bands` and `fit_plane`, the sequences gain analysis steps among the appends, removals, moves, masks,
selections, sorts and writes write_model draws -- so that rtr_select_voxel_grid, rtr_select_neighbours,
rtr_select_clusters, rtr_select_near, rtr_count_in_bands and rtr_fit_plane run on clouds that edits have rewritten in
place, not only on clouds uploaded once.  test_gpu_analysis_sequences.py drives the library with them,
test_analysis_model_host.py checks this file without a GPU.  numpy only.

Results come from the exact references in their brute-force forms alone (voxel_ref.select, neighbours_ref.counts_brute /
select, clusters_ref.labels_brute / hits / stats, near_ref.near_brute / stats, planes_ref.counts / fit,
select_ref.combine), which share no grid with the library.  The one piece of arithmetic written here is `axis_in_span`,
a transcription of neighbour_axis (csrc/rtr_neighbour_cell.h): it predicts RTR_ERR_UNSUPPORTED.

An analysis record: "call" = "analysis"; "kind": one of KINDS; "op" / "outside" as a select record's; the kind's
parameters as plain Python values (a radius is the float of a float32; the given points of `near` are named by a seed
and built by `materialize` on the state before the step, as a mask spec is); "edge": None, "beyond_span" or "at_span";
"state": what the cloud was when the step was drawn -- {"sorted", "chunks", "mixed_scale": some 256-point chunk of upload
order holds points whose generator level or thrown flag differ, "nonfinite": a point has a NaN or infinite coordinate,
"selection": one exists, "selection_by": the call that made it, "after": the call of the previous step, "after_edge":
its edge}.

Parameters are drawn from the model's state before the step in float64 -- a measure to choose by, like pose_for, not a
reference.  When the previous step changed coordinates or the point set, the point q the parameters are built round is
taken next to what that step touched (the moved, written or appended points; the nearest survivors of removed ones), so
that a result computed on the state BEFORE the edit differs from the true one: test_analysis_model_host.py measures
that share."""
import functools

import numpy as np

import clusters_ref as cr
import edit_model as em
import near_ref
import neighbours_ref as nr
import planes_ref
import select_ref
import voxel_ref
import write_model as wm
from edit_model import FAMILIES, pose_for  # noqa: F401  (the GPU file's families and camera are edit_model's)

f32 = np.float32
W, H = em.W, em.H
SEEDS = (1, 2, 3)
STEPS = 30
KINDS = ("voxel", "neighbours", "clusters", "near", "bands", "fit_plane")
SELECTING = ("voxel", "neighbours", "clusters", "near")  # (the kinds that write the selection)
SPAN_STEPS = (("neighbours", "beyond_span"), ("clusters", "at_span"), ("near", "beyond_span"),
              ("neighbours", "at_span"), ("clusters", "beyond_span"), ("near", "at_span"))
# the edges of edit_model an analysis step follows directly ("append_empty" closes remove_all_then_append)
FOLLOWED = ("move_scale_shear", "move_shrink", "move_far", "remove_one_per_chunk", "remove_point_0", "append_to_256",
            "append_past_256", "reorder", "append_empty", "directed_write")
CLUSTER_WINDOWS = ((1, 0), (2, 0), (50, 0), (2, 49))
GIVEN_COUNTS = (0, 1, 63, 64, 65, 700)
# a span step waits for a cloud of more than one chunk and for a step that is no edit (the steps behind an edit are the
# ones drawn next to what it touched), but only up to this step
SPAN_LATEST = 22
CELL_MIN, CELL_MAX = -(2 ** 20 - 1), 2 ** 20 - 2


# ---- the span of the library's internal grid (a transcription of neighbour_axis) --------------------------------------
def cell_edge(radius):
    return np.float64(f32(radius)) * (1.0 + 2.0 ** -10)


def axis_in_span(p, radius):
    """bool, shaped as p: the finite coordinates whose cell floor(float64(p) / h) lies in the span."""
    p = np.asarray(p, f32)
    with np.errstate(all="ignore"):
        q = np.floor(p.astype(np.float64) / cell_edge(radius))
        return np.isfinite(p) & (q >= CELL_MIN) & (q <= CELL_MAX)


def beyond_span(xyz, radius):
    """bool [n]: the points with three finite coordinates of which one has no cell (what the calls refuse)."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    return np.isfinite(xyz).all(axis=1) & ~axis_in_span(xyz, radius).all(axis=1)


def _ok_radius(r):
    with np.errstate(all="ignore"):
        r = f32(r)
        r2 = r * r
    return bool(np.isfinite(r) and r > 0 and np.isfinite(r2) and r2 >= np.finfo(f32).tiny)


# ---- the model ----------------------------------------------------------------------------------------------------------
class Model(wm.Model):
    """write_model.Model with one method per analysis call.  Each returns a dict: "error" (None, "unsupported": the
    facade raises RtrError with RTR_ERR_UNSUPPORTED and nothing changes, or "degenerate": fit_plane's RuntimeError),
    "stats", and the kind's outputs; the selecting kinds also "hit" (before OUTSIDE and op) and update self.selection."""

    def copy(self):
        m = Model(self.family)
        m.__dict__.update(em.Model.copy(self).__dict__)
        return m

    def _combine(self, op, outside, hit):
        sel = np.zeros(self.n, bool) if self.selection is None else self.selection
        self.selection = select_ref.combine(op, sel, ~hit if outside else hit)
        return int(self.selection.sum())

    def voxel(self, cell, origin, min_count, op, outside):
        assert self.n > 0
        hit, st = voxel_ref.select(self.xyz, cell, origin, min_count)
        return {"error": None, "hit": hit, "stats": (self._combine(op, outside, hit),) + st}

    def neighbours(self, radius, min_neighbours, op, outside):
        assert self.n > 0
        if beyond_span(self.xyz, radius).any():
            return {"error": "unsupported"}
        hit, st = nr.select(self.xyz, radius, min_neighbours, nr.counts_brute(self.xyz, radius))
        return {"error": None, "hit": hit, "stats": (self._combine(op, outside, hit),) + st}

    def clusters(self, radius, min_points, max_points, seeded, op, outside):
        assert self.n > 0
        if beyond_span(self.xyz, radius).any():
            return {"error": "unsupported"}
        lab = cr.labels_brute(self.xyz, radius)
        seeds = None
        if seeded:
            seeds = np.zeros(self.n, bool) if self.selection is None else self.selection
        hit = cr.hits(lab, min_points, max_points, seeds)
        st = cr.stats(lab, hit)
        return {"error": None, "hit": hit, "labels": lab, "stats": (self._combine(op, outside, hit),) + st}

    def near(self, G, radius, op, outside, near, given_only):
        assert self.n > 0
        G = np.asarray(G, f32).reshape(-1, 3)
        if beyond_span(G, radius).any():
            return {"error": "unsupported"}
        hit, bits = near_ref.near_brute(self.xyz, G, radius)
        if given_only:  # (the selection is neither read, changed nor created)
            none = np.zeros(self.n, bool)
            return {"error": None, "hit": hit, "near": bits, "stats": near_ref.stats(none, bits, G, none)}
        self._combine(op, outside, hit)
        return {"error": None, "hit": hit, "near": bits if near else None,
                "stats": near_ref.stats(hit, bits if near else None, G, self.selection)}

    def _population(self, selected):
        if not selected:
            return None
        return np.zeros(self.n, bool) if self.selection is None else self.selection

    def bands(self, bands, selected):
        assert self.n > 0
        pop = self._population(selected)
        return {"error": None, "counts": planes_ref.counts(self.xyz, bands, pop),
                "stats": (self.n if pop is None else int(pop.sum()),)}

    def fit_plane(self, dist, iterations, seed, selected):
        assert self.n > 0
        plane, st = planes_ref.fit(self.xyz, dist, iterations, seed, self._population(selected))
        return {"error": "degenerate" if st[1] == 0 else None, "plane": plane, "stats": st}


# ---- step records ---------------------------------------------------------------------------------------------------------
def given_points(rec, model):
    """float32 (m, 3): the given points of a `near` record on the model's state before the step.  Half are finite
    resident points (the ones the record names in given["at"], next to the last edit, where it names some) displaced by
    a uniform offset in [-r, r]^3, r = given["radius"], every eighth of them left exactly coincident; half are an
    edit_model.block of a BOXES entry; given["specials"] values of edit_model.SPECIALS are placed among them."""
    g = rec["given"]
    m, r = g["m"], g["radius"]
    rng = np.random.default_rng(g["data"])
    fin = np.flatnonzero(np.isfinite(model.xyz).all(axis=1))
    k = (m + 1) // 2 if fin.size else 0
    if g["at"] is not None and k:  # (resident points named by the generator: next to what the last edit touched)
        at = np.asarray(g["at"], np.int64)
        idx = at[rng.integers(at.size, size=k)]
    else:
        idx = fin[rng.integers(fin.size, size=k)] if k else np.zeros(0, np.int64)
    with np.errstate(all="ignore"):
        res = model.xyz[idx].astype(np.float64) + rng.uniform(-r, r, size=(k, 3)) * (np.arange(k) % 8 != 0)[:, None]
    blk, _ = em.block({"m": m - k, "data": g["data"], "box": g["box"]})
    G = np.concatenate([res.astype(f32), blk]).astype(f32)
    if m:
        G = G[rng.permutation(m)]
        for s in range(min(g["specials"], m)):
            G[rng.integers(m), rng.integers(3)] = em.SPECIALS[rng.integers(em.SPECIALS.size)]
    return np.ascontiguousarray(G.reshape(m, 3))


def materialize(rec, model):
    if rec["call"] != "analysis":
        return wm.materialize(rec, model)
    kind = rec["kind"]
    if kind == "near":
        return {"G": given_points(rec, model)}
    if kind == "bands":
        return {"bands": np.array(rec["bands"], f32).reshape(-1, 5)}
    return {}


def analyse(model, rec, args):
    """The record's call on the model: the result dict of Model's method."""
    kind = rec["kind"]
    if kind == "voxel":
        return model.voxel(rec["cell"], rec["origin"], rec["min_count"], rec["op"], rec["outside"])
    if kind == "neighbours":
        return model.neighbours(rec["radius"], rec["min_neighbours"], rec["op"], rec["outside"])
    if kind == "clusters":
        return model.clusters(rec["radius"], rec["min_points"], rec["max_points"], rec["seeded"], rec["op"], rec["outside"])
    if kind == "near":
        return model.near(args["G"], rec["radius"], rec["op"], rec["outside"], rec["near"], rec["given_only"])
    if kind == "bands":
        return model.bands(args["bands"], rec["selected"])
    if kind == "fit_plane":
        return model.fit_plane(rec["dist"], rec["iterations"], rec["seed"], rec["selected"])
    raise ValueError(kind)


def apply(model, rec, args):
    """-> the analysis result, or None for every other call."""
    if rec["call"] != "analysis":
        return wm.apply(model, rec, args)
    return analyse(model, rec, args)


def trivial(rec, res, n):
    """Does an analysis step that succeeded say nothing?  (The rule of the host test's "not trivial" condition.)"""
    kind = rec["kind"]
    if kind in ("voxel", "neighbours", "near"):
        return int(res["hit"].sum()) in (0, n)
    if kind == "clusters":
        return res["stats"][1] in (1, n)
    if kind == "bands":
        return bool(np.isin(res["counts"], (0, n)).all())
    return False


class _Gen(wm._Gen):
    def __init__(self, seed, family):
        super().__init__(seed, family)
        self.model = Model(family)
        self.arng = np.random.default_rng([seed, sorted(FAMILIES).index(family), 3])  # (the analysis steps' own chain)
        self.kind_k = 2 * seed  # (the seeds start the rotation at different kinds)
        # the edges an analysis step follows come first, so that a sequence of STEPS steps reaches them: appends and the
        # three moves that leave a chunk of mixed scales in turn, from a seed-dependent start, the removal of every
        # point, which ends that state, in their middle
        first = ["append_to_256", "move_scale_shear", "remove_point_0", "move_shrink", "append_past_256", "move_far",
                 "remove_one_per_chunk", "reorder"]
        first = [e for e in first[2 * seed % 8:] + first[:2 * seed % 8] if e in self.todo]
        first.insert(4, "remove_all_then_append")
        self.todo = first + [e for e in self.todo if e not in first]
        self.calls = {k: 0 for k in KINDS}
        self.met = {k: set() for k in KINDS}
        self.fair = {k: 0 for k in KINDS}  # (the steps of the rotation alone: span steps are extra)
        self.seed = seed
        self.empty_done = set()
        # the kinds still to run on a selection that is there: `selected` bands and fit_plane, seeded clusters
        self.sel_need = (["bands", "fit_plane", "clusters"] * 2)[seed % 3:seed % 3 + 3]
        self.span_todo = list(SPAN_STEPS[seed % len(SPAN_STEPS):] + SPAN_STEPS[:seed % len(SPAN_STEPS)])
        self.span_owed = 0
        self.follow = False        # the last step was one of FOLLOWED: an analysis step comes next
        self.hot = None            # float64 (k, 3): where the last edit changed the cloud
        self.touched = None        # bool (n,): the points it wrote (None: none of those resident, or all)
        self.prev = (None, None)   # (call, edge) of the last step
        self.selection_by = None   # the call that made the selection in force

    # -- drawing parameters
    def _finite(self):
        return np.flatnonzero(np.isfinite(self.model.xyz).all(axis=1))

    def _near_hot(self, count, dist=None):
        """Upload indices of `count` finite points: random ones, or, where the last edit changed the cloud, the points
        nearest to random hot positions -- among the points that edit left alone where there are some (the seam between
        the old and the new).  dist: a list that receives each one's distance to its hot position."""
        fin = self._finite()
        if self.hot is None or not len(self.hot):
            return fin[self.arng.integers(fin.size, size=count)]
        if self.touched is not None and not self.touched[fin].all():
            fin = fin[~self.touched[fin]]
        p = self.model.xyz[fin].astype(np.float64)
        out = []
        for h in self.hot[self.arng.integers(len(self.hot), size=count)]:
            d2 = ((p - h) ** 2).sum(axis=1)
            out.append(fin[int(np.argmin(d2))])
            if dist is not None:
                dist.append(float(np.sqrt(d2.min())))
        return np.array(out, np.int64)

    def _radius(self, kmax=16, rank=None):
        """(radius, q, k): float32(1.0001 x the distance from a finite point q to its k-th nearest finite point), k in
        {1, 4, 16} and at most kmax (or `rank`, where nearest_model.py names one: nothing is drawn for k then); None where
        the cloud has no such radius whose square is a normal float32.  Where q was taken next to a hot position, the
        distance is stretched to reach that position if eight times it does."""
        fin = self._finite()
        if fin.size < 2:
            return None
        p = self.model.xyz[fin].astype(np.float64)
        for _ in range(16):
            reach = []
            i = int(self._near_hot(1, reach)[0])
            q = self.model.xyz[i].astype(np.float64)
            k = max(1, min(int(self.arng.choice([1, 4, 16])) if rank is None else rank, fin.size - 1, kmax))
            d = np.sqrt(np.sort(((p - q) ** 2).sum(axis=1))[k])  # ([0] is q itself)
            if reach and d < reach[0] <= 8 * d:
                d = reach[0]
            with np.errstate(all="ignore"):
                r = f32(1.0001 * d)
            if _ok_radius(r):
                return float(r), q, k
        return None

    def _largest(self, xyz):
        xyz = np.asarray(xyz, f32).reshape(-1, 3)
        fin = xyz[np.isfinite(xyz).all(axis=1)]
        return float(np.abs(fin.astype(np.float64)).max()) if fin.size else 0.0

    def _span_radius(self, xyz, edge):
        """The radius of a directed span step on the points xyz, or None where they allow none."""
        r = f32((0.99 if edge == "beyond_span" else 1.01) * self._largest(xyz) / 2.0 ** 20)
        if not _ok_radius(r):
            return None
        return float(r) if beyond_span(xyz, r).any() == (edge == "beyond_span") else None

    def _op(self):
        return em.OPS[int(self.arng.integers(len(em.OPS)))], bool(self.arng.random() < 0.3)

    def _state(self):
        mo, n = self.model, self.model.n
        pad = (-n) % em.CHUNK
        lv = np.concatenate([self.level.astype(np.int64) * 2 + self.thrown, np.full(pad, -99)]).reshape(-1, em.CHUNK)
        real = lv != -99
        lo = np.where(real, lv, 99).min(axis=1)
        hi = np.where(real, lv, -99).max(axis=1)
        return {"sorted": bool(mo.sorted), "chunks": (n + em.CHUNK - 1) // em.CHUNK, "mixed_scale": bool((lo != hi).any()),
                "nonfinite": bool(not np.isfinite(mo.xyz).all()), "selection": mo.selection is not None,
                "selection_by": self.selection_by if mo.selection is not None else None,
                "after": self.prev[0], "after_edge": self.prev[1]}

    def _given(self, radius, m=None):
        a = self.arng
        m = int(a.choice(GIVEN_COUNTS)) if m is None else m
        at = None
        if self.hot is not None and len(self.hot) and self._finite().size:
            at = [int(v) for v in self._near_hot(min(16, max(1, m)))]
        return {"m": m, "radius": radius, "data": int(a.integers(1 << 30)), "box": int(a.integers(len(em.BOXES))), "at": at,
                "specials": int(a.integers(1, 4)) if self.special else 0}

    def _analysis(self, kind, edge=None, selected=None):
        """The record of an analysis step of `kind` on the current state, or None where the cloud allows none."""
        mo, a = self.model, self.arng
        if mo.n == 0:
            return None
        k = self.calls[kind] + self.seed  # (the alternations of a kind start differently in every seed)
        op, outside = self._op()
        rec = {"call": "analysis", "kind": kind, "op": op, "outside": outside, "edge": edge}
        if kind in ("bands", "fit_plane") or (kind == "near" and k % 4 == 3 and edge is None):
            rec["op"], rec["outside"] = "replace", False  # (they leave the selection alone)
        # (clusters: the k-th neighbour's distance joins a uniform block of a few hundred points into ONE cluster unless
        # k is small against the block, so k is at most 1 below 1024 points, 4 below 4096)
        rq = self._radius(max(1, mo.n // 256) if kind == "clusters" else 16)
        if kind in ("neighbours", "clusters"):
            if edge is not None:
                r = self._span_radius(mo.xyz, edge)
            else:
                r = rq[0] if rq else None
            if r is None:
                return None
            rec["radius"] = r
            if kind == "neighbours":
                # (at most the k of the radius, so that q itself hits: never an empty result by construction)
                rec["min_neighbours"] = int(a.choice([v for v in (1, 4, 16) if edge is not None or v <= max(1, rq[2])]))
            else:
                lo, hi = CLUSTER_WINDOWS[int(a.integers(len(CLUSTER_WINDOWS)))]
                rec.update(min_points=lo, max_points=hi, seeded=bool(k % 2) if selected is None else selected, labels=True)
        elif kind == "voxel":
            if rq is None:
                return None
            r, q = rq[:2]
            scale = (2.0,) if k % 2 == 0 else (2.0, 3.0, 1.5)
            with np.errstate(all="ignore"):
                cell = [f32(s * r) for s in scale]
                origin = [f32(q[j] - a.random() * float(cell[j % len(cell)])) for j in range(3)]
                good = all(np.isfinite(c) and c > 0 and np.isfinite(f32(1) / c) for c in cell) and np.isfinite(origin).all()
            if not good:
                return None
            rec.update(cell=float(cell[0]) if len(cell) == 1 else [float(c) for c in cell],
                       origin=[float(o) for o in origin], min_count=int(a.choice([1, 2, 5])))
        elif kind == "near":
            rec.update(near=bool(k % 2 == 1), given_only=bool(k % 4 == 3 and edge is None),
                       source=("host", "device")[k % 2], width=(3, 4)[(k // 2) % 2])
            if edge is not None:  # (the offsets of the resident half keep a drawn radius; the call's is the span's)
                if rq is None:
                    return None
                rec["given"] = self._given(rq[0], 63)
                rec["radius"] = self._span_radius(given_points(rec, mo), edge)
                if rec["radius"] is None:
                    return None
            else:
                for t in range(8):  # (redrawn while a finite given point is beyond the span)
                    if t:
                        rq = self._radius()
                    if rq is None:
                        return None
                    rec["radius"], rec["given"] = rq[0], self._given(rq[0])
                    if not beyond_span(given_points(rec, mo), rq[0]).any():
                        break
                else:
                    return None
        elif kind == "bands":
            sel = self._selected(kind, bool(k % 2), selected)
            bands = self._bands(int((1, 64, 65)[k % 3]), k, sel)
            if bands is None:
                return None
            rec.update(bands=bands, selected=sel)
        elif kind == "fit_plane":
            if rq is None:
                return None
            rec.update(dist=rq[0], iterations=int((16, 65)[k % 2]), seed=int(a.integers(1 << 62)) * 4 + int(a.integers(4)),
                       selected=self._selected(kind, bool((k // 2) % 2), selected))
        else:
            raise ValueError(kind)
        self.calls[kind] += edge is None  # (the alternations go through the steps that are no span steps)
        rec["state"] = self._state()
        return rec

    def _selected(self, kind, want, forced=None):
        """`selected` of a bands / fit_plane step: alternating, but without a selection only once per kind, in the
        sequences of one seed (the population is empty then, and every answer is zero)."""
        if forced is not None:
            return forced
        if want and self.model.selection is not None and not self.model.selection.any():
            return False
        if want and self.model.selection is None:
            if kind in self.empty_done or self.seed != {"bands": SEEDS[0], "fit_plane": SEEDS[1]}[kind]:
                return False
            self.empty_done.add(kind)
        return want

    def _bands(self, count, k, selected):
        """`count` bands as lists of floats: planes_ref.band_of a plane through three finite resident points (one of them
        next to the last edit, one a selected point when only those are counted) with distance 0, a radius or 100
        radii, and one axis-aligned band that holds every finite point of one 256-point chunk of upload order."""
        mo, a = self.model, self.arng
        fin = self._finite()
        if fin.size < 3:
            return None
        out = []
        pop = fin
        if selected and mo.selection is not None and mo.selection[fin].any():
            pop = fin[mo.selection[fin]]
        c = int(a.integers((mo.n + em.CHUNK - 1) // em.CHUNK))
        part = mo.xyz[c * em.CHUNK:(c + 1) * em.CHUNK]
        part = part[np.isfinite(part).all(axis=1)]
        ax = int(a.integers(3))
        if len(part) and (count > 1 or (k % 2 == 0 and mo.n > em.CHUNK)):  # (alone only where it is not every point)
            nrm = [0.0, 0.0, 0.0]
            nrm[ax] = 1.0
            band = np.array(nrm + [-float(part[:, ax].min()), float(part[:, ax].max())], f32)
            if np.isfinite(band).all():
                out.append([float(v) for v in band])
        tries = 0
        while len(out) < count and tries < 4 * count + 16:
            tries += 1
            rq = self._radius()
            if rq is None:
                return None
            i = [int(self._near_hot(1)[0]), int(pop[a.integers(pop.size)]), int(fin[a.integers(fin.size)])]
            pl = planes_ref.candidate(mo.xyz[i[0]], mo.xyz[i[1]], mo.xyz[i[2]], i)
            if pl is None:
                continue
            band = planes_ref.band_of(pl, f32(rq[0]) * f32((0.0, 1.0, 100.0)[tries % 3]))
            if np.isfinite(band).all():
                out.append([float(v) for v in band])
        if len(out) < count:
            return None
        pos = int(a.integers(count))
        out[0], out[pos] = out[pos], out[0]  # (the axis-aligned band anywhere among them)
        return out

    def _flags(self):
        st = self._state()
        return {k for k in ("mixed_scale", "sorted", "nonfinite") if st[k]} | ({"chunks"} if st["chunks"] >= 3 else set())

    def _next_analysis(self, edge=None, kind=None):
        """The next analysis step: of `kind`; or, while a selection of three points or more is there, of a kind that has
        yet to run on one (sel_need); or of the kinds in rotation the one that has not met the most of the states the
        cloud is in now (three chunks or more, a chunk of mixed scales, sorted, non-finite points)."""
        if kind is not None:
            return self._analysis(kind, edge)
        if self.sel_need and self.model.selection is not None and self.model.selection.sum() >= 3:
            rec = self._analysis(self.sel_need[0], edge, selected=True)
            if rec is not None:
                self.fair[self.sel_need.pop(0)] += 1
                return rec
        now = self._flags()
        order = [KINDS[(self.kind_k + 1 + j) % len(KINDS)] for j in range(len(KINDS))]
        turn = lambda k: (KINDS.index(k) - 2 * self.seed) % len(KINDS)  # noqa: E731  (every seed serves other kinds first)
        order.sort(key=lambda k: (-len(now - self.met[k]), turn(k) if now - self.met[k] else 0, self.fair[k]))
        for k in order:
            rec = self._analysis(k, edge)
            if rec is not None:
                self.kind_k = KINDS.index(k)
                self.fair[k] += 1
                self.met[k] |= now
                return rec
        return None

    def _random(self):
        if self.model.n > 0 and self.arng.random() < 0.33:
            rec = self._next_analysis()
            if rec is not None:
                return rec
        return super()._random()

    # -- what the last edit touched
    def _note(self, rec, args, before):
        mo, call = self.model, rec["call"]
        hot = touched = None
        if call in ("upload", "append"):
            hot = args["xyz"]
            if call == "append" and 0 < before.n < mo.n:
                touched = np.arange(mo.n) >= before.n
        elif call == "remove":
            hot = before.xyz[~args["bits"]]
        elif call == "transform":
            hot = mo.xyz if args["bits"] is None else mo.xyz[args["bits"]]
            touched = args["bits"]
        elif call == "write" and args["X"] is not None:
            bits = np.ones(before.n, bool) if args["bits"] is None else args["bits"]
            idx = np.flatnonzero(bits)[args["first"]:args["first"] + args["X"].shape[0]]
            hot, touched = mo.xyz[idx], np.zeros(mo.n, bool)
            touched[idx] = True
        if call != "analysis":
            self.touched = touched if mo.n else None
            if hot is not None:
                hot = np.asarray(hot, np.float64).reshape(-1, 3)
                hot = hot[np.isfinite(hot).all(axis=1)]
            self.hot = hot if hot is not None and len(hot) else None
        if call == "select" or (call == "analysis" and rec["kind"] in SELECTING):
            if mo.selection is not None and not (call == "analysis" and rec.get("given_only")):
                self.selection_by = call if call == "select" else rec["kind"]
        self.follow = rec["edge"] in FOLLOWED and call != "analysis"
        if call == "analysis" and rec["kind"] in SELECTING and self.sel_need and mo.selection is not None and \
                mo.selection.sum() >= 3:
            self.follow = True  # (a selection an analysis step made: the next step counts or fits what it holds)
        self.prev = (call if call != "analysis" else rec["kind"], rec["edge"])

    def step(self, i):
        """write_model._Gen.step with, in front of it, the analysis step that follows an edge of FOLLOWED directly, and,
        behind the directed writes, the steps of SPAN_STEPS (one is owed at every fourth step from step 5 on)."""
        rec, mo = None, self.model
        if i == 0:
            rec = self._block("upload", int(self.rng.choice(em.START_COUNTS)))
        self.owed += i % 3 == 2 or i % 6 == 3  # (half the steps: the followed edges all fit into STEPS steps)
        self.span_owed += i % 4 == 1 and i >= 5
        if rec is None and self.follow:
            rec = self._next_analysis()
        if rec is None and not self.forced and i >= 2:  # upkeep: the states the coverage asks for do not last by themselves
            if 0 < mo.n <= 3 * em.CHUNK and i % 2 == 0:  # (a removal or an upload has left fewer than four chunks)
                rec = self._block("append", int(self.arng.integers(3 * em.CHUNK + 1, 3000)))
            elif em.allows_reorder(self.family) and not mo.sorted and mo.n >= 2 and i >= 6 and i % 3 == 0:
                rec = {"call": "reorder", "edge": None}  # (an upload or an emptied context has lost the sort)
        if rec is None and not self.forced and mo.n >= 2 * em.CHUNK and (i in (7, 13, 19) or self.write_due):
            if mo.keep is None:
                rec, self.write_due = self._keep(("random", self._seed(), 0.8)), True
            elif i >= 13 and em.allows_reorder(self.family) and not mo.sorted:  # (the later ones on a sorted cloud)
                rec, self.write_due = {"call": "reorder", "edge": None}, True
            else:
                rec, self.write_due = self._write(("range", 3, em.CHUNK + 9), 0.0, 1.0, ("both", "xyz", "rgb")[i % 3]), False
                rec["edge"] = "directed_write"
        while rec is None and self.forced:
            rec = self._forced(self.forced.pop(0))
        settled = self.prev[0] in KINDS + ("set_keep", "clear_keep", "select")  # (the last step left the points alone)
        if rec is None and self.span_owed and self.span_todo and ((mo.n > em.CHUNK and settled) or i >= SPAN_LATEST):
            for s in list(self.span_todo):
                rec = self._next_analysis(s[1], s[0])
                if rec is not None:
                    self.span_owed -= 1
                    self.span_todo.remove(s)
                    break
        if rec is None and self.owed and self.todo:
            for e in list(self.todo):
                rec = self._edge(e)
                if rec is not None:
                    self.owed -= 1
                    self.todo.remove(e)
                    if e in ("append_empty", "remove_all_then_append"):  # (one pair of steps covers both)
                        for o in ("append_empty", "remove_all_then_append"):
                            if o in self.todo:
                                self.todo.remove(o)
                    break
        if rec is None:
            rec = self._random()
        before = mo.copy()
        args, n0 = materialize(rec, mo), mo.n
        res = apply(mo, rec, args)
        if rec["call"] != "analysis":
            self._track(rec, args, n0)
        self._note(rec, args, before)
        assert mo.n <= em.N_MAX and self.level.shape == self.thrown.shape == (mo.n,)
        self.done = (rec, args, res, n0, before.selection, None if mo.selection is None else mo.selection.copy())
        return rec


@functools.lru_cache(maxsize=None)
def replay(seed, family, steps=STEPS):
    """[(record, arguments, result, n before, selection before, selection after)] of the sequence on the model alone, a
    pure function of the arguments (result: None for a step that is no analysis).  The references are computed once,
    while the sequence is drawn, and shared by every test that needs them: cached, read, never changed."""
    g, out = _Gen(int(seed), family), []
    for i in range(steps):
        g.step(i)
        out.append(g.done)
    return tuple(out)


def sequence(seed, family, steps=STEPS):
    """`steps` step records: write_model.sequence's calls with analysis steps among them."""
    return tuple(r[0] for r in replay(seed, family, steps))


def frame_steps(steps):
    return em.frame_steps(steps)


# Regressions: prefixes of random sequences that failed on the library, as literal steps: {name: (family, [records])}.
REGRESSIONS = {}
