"""analysis_model.py with the nearest-point queries in it (include/rtr.h sections 6l and 6m): `Model` gains `nearest`,
`nearest_k` and `merge` (ProjectCloud.appendNewPoints), the sequences gain query steps among the appends, removals,
moves, masks, selections, sorts and writes write_model draws -- so that rtr_nearest_points and rtr_nearest_k_points, which
RETURN upload indices, distance bits and ranks, run on clouds that edits have rewritten in place and whose indices
removals have renumbered.  test_gpu_nearest_sequences.py drives the library with them, test_nearest_model_host.py checks
this file without a GPU.  numpy only.

Results come from the brute-force references alone (nearest_ref.nearest_brute, nearest_k_ref.nearest_k_brute,
near_ref.near_brute), which share no grid with the library; analysis_model.beyond_span predicts RTR_ERR_UNSUPPORTED.

Records.  A query: "call" = "query"; "kind": "nearest" or "nearest_k"; "radius"; "given": the spec of the given points
(analysis_model.given_points'; with "all_at" every point lies at or within the radius of one of the resident points
at[0] .. at[1] - 1, every eighth coincident; {"ref": i} names the given points of step i of the same sequence, the one
place where a record reuses arrays of an earlier step: the ICP step, whose points were built BEFORE the move); "source" /
"width": host or device rows of 3 or 4 floats; nearest: "outputs" ("given", "resident" or "both") and "match" (through
ProjectCloud.matchPoints); nearest_k: "k"; "edge": None, "beyond_span", "at_span", or the name of the directed query;
"state": analysis_model's, with "n" and "finite", the number of points and of finite ones.
A merge: "call" = "merge"; "radius", "given", "data" (the seed of the colours).
"append_copies": appends exact copies (coordinates bit for bit, colours of their own) of "count" finite resident points
the seed chooses, the first third of them twice.  "remove_originals": removes the points an append_copies record with the
same "seed" and "count" copied from the first "base" points -- the lower-indexed member of every copied pair.
Every other record is write_model's."""
import functools

import numpy as np

import analysis_model as am
import edit_model as em
import near_ref
import nearest_k_ref
import nearest_ref
import write_model as wm
from analysis_model import FAMILIES, axis_in_span, beyond_span, pose_for  # noqa: F401
from nearest_ref import NONE

f32 = np.float32
SEEDS = (1, 2, 3)
STEPS = 30
QUERIES = ("nearest", "nearest_k")
NEW = QUERIES + ("merge",)
KS = (1, 2, 8, 64)
OUTPUTS = ("given", "resident", "both")
GIVEN_COUNTS = am.GIVEN_COUNTS
GIVEN_ROTATION = (700, 64, 63, 65, 1, 700, 64, 0, 65, 63)  # (no given points at all: a tenth of the random queries)
TIE_COUNTS = (700, 257, 385)  # (the given counts of the directed tie queries: 88, 33 and 49 coincident points)
SPAN_STEPS = (("nearest", "beyond_span"), ("nearest_k", "at_span"), ("nearest_k", "beyond_span"), ("nearest", "at_span"))
# the edits of edit_model / write_model a query follows directly, a third of them in the sequences of every seed
FOLLOWED = am.FOLLOWED
SHARED = ("append_to_256", "remove_all_then_append", "remove_point_0", "move_shrink", "move_scale_shear", "directed_write",
          "remove_one_per_chunk", "append_past_256", "move_far")
DIRECTED = ("append_copies", "remove_originals", "append_copies_sorted", "reorder", "icp_move")
EMPTY_APPEND = (300, 37, 255)  # (the points behind a removal of every point, by seed: 37 are fewer than k = 64)


# ---- the model ----------------------------------------------------------------------------------------------------------
class Model(am.Model):
    """analysis_model.Model with the two queries and the merge.  Each returns a dict: "error" (None or "unsupported":
    the facade raises RtrError with RTR_ERR_UNSUPPORTED and nothing changes) and the call's outputs."""

    def copy(self):
        m = Model(self.family)
        m.__dict__.update(em.Model.copy(self).__dict__)
        return m

    def nearest(self, G, radius, given=True, resident=False):
        assert self.n > 0
        G = np.asarray(G, f32).reshape(-1, 3)
        if beyond_span(G, radius).any():
            return {"error": "unsupported"}
        gi, gd, ri, rd, st = nearest_ref.nearest_brute(self.xyz, G, radius)
        return {"error": None, "all": (gi, gd, ri, rd), "given": (gi, gd) if given else None,
                "resident": (ri, rd) if resident else None, "stats": st}

    def nearest_k(self, G, radius, k):
        assert self.n > 0
        G = np.asarray(G, f32).reshape(-1, 3)
        if beyond_span(G, radius).any():
            return {"error": "unsupported"}
        idx, d2, found, st = nearest_k_ref.nearest_k_brute(self.xyz, G, radius, k)
        return {"error": None, "index": idx, "dist2": d2, "found": found, "stats": st}

    def merge(self, G, C, radius):
        """ProjectCloud.appendNewPoints: the given points without a resident point within the radius are appended, in
        their order.  A given point that is not finite is near nothing, so its near bit is clear and the facade appends
        it like every other new point: so does the model."""
        assert self.n > 0
        G = np.asarray(G, f32).reshape(-1, 3)
        if beyond_span(G, radius).any():
            return {"error": "unsupported"}
        new = ~near_ref.near_brute(self.xyz, G, radius)[1]
        if new.any():
            self.append(G[new], np.asarray(C, np.uint8).reshape(-1, 3)[new])  # (the selection goes, as with any append)
        return {"error": None, "new": new, "appended": int(new.sum())}


# ---- step records ---------------------------------------------------------------------------------------------------------
def given_points(rec, model, past=None):
    """float32 (m, 3): the given points of a query or merge record on the model's state before the step (past: the
    arguments of the sequence's earlier steps, for a spec that names one)."""
    g = rec["given"]
    if "ref" in g:
        return past[g["ref"]]["G"]
    if not g.get("all_at"):
        return am.given_points(rec, model)
    m, r = g["m"], g["radius"]
    rng = np.random.default_rng(g["data"])
    idx = rng.integers(g["at"][0], g["at"][1], size=m)
    off = rng.uniform(-0.55 * r, 0.55 * r, size=(m, 3)) * (np.arange(m) % 8 != 0)[:, None]  # (|off| < r; every eighth: none)
    with np.errstate(all="ignore"):
        G = (model.xyz[idx].astype(np.float64) + off).astype(f32)
    for s in range(min(g["specials"], m)):
        G[rng.integers(m), rng.integers(3)] = em.SPECIALS[rng.integers(em.SPECIALS.size)]
    return np.ascontiguousarray(G.reshape(m, 3))


def copied(rec, xyz):
    """Upload indices of the points an append_copies record copies from the points xyz, in the order of the copies."""
    fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    idx = np.random.default_rng(rec["seed"]).permutation(fin)[:rec["count"]]
    return np.concatenate([idx, idx[:idx.size // 3]])


def materialize(rec, model, past=None):
    call = rec["call"]
    if call == "query":
        return {"G": given_points(rec, model, past)}
    if call == "merge":
        G = given_points(rec, model, past)
        return {"G": G, "C": np.random.default_rng(rec["data"]).integers(0, 256, size=(G.shape[0], 3)).astype(np.uint8)}
    if call == "append_copies":
        src = copied(rec, model.xyz)
        rgb = np.random.default_rng(rec["seed"] + 1).integers(0, 256, size=(src.size, 3)).astype(np.uint8)
        return {"xyz": model.xyz[src].copy(), "rgb": rgb, "src": src}
    if call == "remove_originals":
        bits = np.ones(model.n, bool)
        bits[copied(rec, model.xyz[:rec["base"]])] = False
        return {"bits": bits}
    return wm.materialize(rec, model)


def apply(model, rec, args):
    """-> the result of a query or merge, None for every other call."""
    call = rec["call"]
    if call == "query":
        if rec["kind"] == "nearest":
            return model.nearest(args["G"], rec["radius"], rec["outputs"] != "resident", rec["outputs"] != "given")
        return model.nearest_k(args["G"], rec["radius"], rec["k"])
    if call == "merge":
        return model.merge(args["G"], args["C"], rec["radius"])
    if call == "append_copies":
        return model.append(args["xyz"], args["rgb"])
    if call == "remove_originals":
        return model.remove(args["bits"])
    return wm.apply(model, rec, args)


def trivial(rec, res):
    """Does a query or merge that succeeded say nothing?  (The rule of the host test's "not trivial" condition.)"""
    if rec["call"] == "merge":
        return res["appended"] in (0, len(res["new"]))
    if rec["kind"] == "nearest":
        return not (res["all"][0] != NONE).any()
    return not (res["found"] >= min(2, rec["k"])).any()


def outputs(rec, res):
    """What the record's call returns, by name, from the model's result: the arrays that were asked for and the stats."""
    if rec["call"] == "merge":
        return {"appended": res["appended"]}
    out = {"stats": tuple(int(v) for v in res["stats"])}
    if rec["kind"] == "nearest_k":
        out.update(index=res["index"], dist2=res["dist2"], found=res["found"])
        return out
    for side in ("given", "resident"):
        if res[side] is not None:
            out[side + "_index"], out[side + "_dist2"] = res[side]
    return out


def mismatches(got, want):
    """The names under which two dicts of `outputs` differ: arrays by dtype, shape and bits (a distance as its uint32
    view), everything else by value.  The one comparison of the GPU file; the host file hands it altered references."""
    bad = sorted(set(got) ^ set(want))
    for k in sorted(set(got) & set(want)):
        x, y = got[k], want[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
                bad.append(k)
        elif x != y:
            bad.append(k)
    return bad


class _Gen(am._Gen):
    """analysis_model._Gen's parameter rules (_radius, _given, _near_hot, _state) under a step rule of its own: thirty
    steps do not hold every followed edit, the span steps and the chains of copies with a query behind each, so a
    sequence works through an agenda of chains and draws random steps between them."""

    def __init__(self, seed, family):
        super().__init__(seed, family)
        self.model = Model(family)
        fam = sorted(FAMILIES).index(family)
        self.qrng = np.random.default_rng([seed, fam, 4])  # (the query steps' own chain)
        self.qcalls = {k: 0 for k in NEW}
        self.qmet = {k: set() for k in QUERIES}
        self.qfair = {k: 0 for k in NEW}
        self.new_k = seed
        self.given_k = 3 * seed + fam
        self.past = []
        self.queue = []  # the rest of the chain of directed steps in progress
        mine = [e for j, e in enumerate(SHARED) if j % 3 == seed % 3]
        sort = ["sorted"] if em.allows_reorder(family) else []
        spans = [("span",) + s for s in SPAN_STEPS[seed % 4:] + SPAN_STEPS[:seed % 4]]
        # the agenda: chains of directed steps, a query behind every edit of them, in the order they are started
        # (the move, the ICP step and the merge leave the point count alone until the merge appends: one `select` in
        # front of them is in force at every query of theirs, and the merge is seen to drop it)
        move = [e for e in mine if e.startswith("move_")]
        rest = [e for e in mine if not e.startswith("move_")]
        self.agenda = [("edge", rest[0]), ("copies",), spans[0], ("selected", move[0]), spans[1], ("edge", rest[1])] + \
                      [(s,) for s in sort] + [spans[2], spans[3]]
        self.k_rot = seed + fam  # (the rotation of k: the directed queries name their own and leave it alone)
        self.recs = []
        self.left = None
        self.done_new = None

    # -- the records of the new steps
    def _qstate(self):
        st = self._state()
        st.update(n=self.model.n, finite=int(self._finite().size))
        return st

    def _pick(self, kinds):
        """Of `kinds` in rotation the one that has met the fewest of the states the cloud is in now (a merge meets
        none: it takes its turn)."""
        now = self._flags()
        order = [NEW[(self.new_k + 1 + j) % len(NEW)] for j in range(len(NEW))]
        order = [k for k in order if k in kinds]
        order.sort(key=lambda k: (-len(now - self.qmet[k]) if k in QUERIES else 0, self.qfair[k]))
        return order

    def _count(self):
        self.given_k += 1
        return GIVEN_ROTATION[self.given_k % len(GIVEN_ROTATION)]

    def _query(self, kind, edge=None, ties=None, outputs=None, k=None):
        """The record of a query of `kind` on the current state, or None where the cloud allows none.  ties: (lo, hi),
        the resident points every given point lies at or next to."""
        mo, fin = self.model, self._finite().size
        if mo.n == 0:
            return None
        span = edge in ("beyond_span", "at_span")
        c = self.qcalls[kind] + self.seed  # (the alternations of a kind start differently in every seed)
        rec = {"call": "query", "kind": kind, "edge": edge, "source": ("host", "device")[c % 2], "width": (3, 4)[(c // 2) % 2]}
        rank = None
        if kind == "nearest":
            match = c % 3 == 2 and outputs is None and not span
            rec.update(outputs="given" if match else outputs or OUTPUTS[(c - (c + 1) // 3) % 3], match=match)
        else:
            rec["k"] = KS[self.k_rot % 4] if k is None else k
            if 0 < fin < 64 and k is None:
                rec["k"] = 64  # (more than there are points to find)
            rotated = k is None and not span and not 0 < fin < 64
            # (the radius reaches as many neighbours as a row has entries: full rows and partly filled ones)
            rank = rec["k"] if rec["k"] > 1 else None
        if ties is not None:
            rank = max(rank or 4, 4)  # (the copies lie at distance zero)
        if span:  # (the offsets of the resident half keep a drawn radius; the call's is the span's)
            rq = self._radius()
            if rq is None:
                return None
            rec["given"] = self._given(rq[0], 63)
            rec["radius"] = self._span_radius(given_points(rec, mo), edge)
            if rec["radius"] is None:
                return None
        else:
            for t in range(8):  # (redrawn while a finite given point is beyond the span)
                rq = self._radius(64, rank) if rank else self._radius()
                if rq is None:
                    return None
                rec["radius"] = rq[0]
                if ties is None:
                    rec["given"] = self._given(rq[0], self._count() if t == 0 else 64)
                else:
                    rec["given"] = {"m": TIE_COUNTS[c % 3], "radius": rq[0], "data": int(self.qrng.integers(1 << 30)),
                                    "at": [int(ties[0]), int(ties[1])], "all_at": True,
                                    "specials": int(self.qrng.integers(1, 4)) if self.special else 0}
                if not beyond_span(given_points(rec, mo), rq[0]).any():
                    break
            else:
                return None
        self.qcalls[kind] += not span
        if kind == "nearest_k":
            self.k_rot += rotated  # (a slot is used up by a step that succeeds with the rotation's own k only)
        rec["state"] = self._qstate()
        return rec

    def _next_query(self, kinds=QUERIES, **kw):
        for kind in self._pick(kinds):
            rec = self._merge() if kind == "merge" else self._query(kind, **kw)
            if rec is not None:
                self.new_k = NEW.index(kind)
                self.qfair[kind] += 1
                if kind in QUERIES:
                    self.qmet[kind] |= self._flags()
                return rec
        return None

    def _merge(self):
        mo = self.model
        m = (63, 700, 64, 65)[(self.qcalls["merge"] + self.seed) % 4]
        if mo.n == 0 or mo.n + m > em.N_MAX:
            return None
        for t in range(8):
            rq = self._radius(rank=1)  # (a point's nearest neighbour: a larger radius leaves no point of the block half new)
            if rq is None:
                return None
            # (the resident half within 0.55 radius on every axis: half of the given points are no new points)
            rec = {"call": "merge", "radius": rq[0], "given": self._given(0.55 * rq[0], m), "data": int(self.qrng.integers(1 << 30)),
                   "edge": None}
            if not beyond_span(given_points(rec, mo), rq[0]).any():
                break
        else:
            return None
        self.qcalls["merge"] += 1
        rec["state"] = self._qstate()
        self.queue.insert(0, ("query",))
        return rec

    def _copies(self, edge):
        mo = self.model
        fin = self._finite().size
        count = int(self.qrng.integers(64, 301))
        if fin < count or mo.n + count + count // 3 > em.N_MAX:
            return None
        return {"call": "append_copies", "seed": int(self.qrng.integers(1 << 30)), "count": count, "edge": edge}

    # -- the chains
    def _start(self, item):
        """The first record of an agenda item, the rest of its chain in self.queue; None where the cloud allows none."""
        mo, what = self.model, item[0]
        big = mo.n > 3 * em.CHUNK
        if what == "selected":  # (a selection, then the steps that leave it in force, then the merge that drops it)
            if not big:
                return None
            self._then(("edge", item[1]), ("icp",), ("merge",))
            return dict(self._random_select(), edge="selection")
        if what == "span":
            return self._query(item[1], item[2]) if mo.n > em.CHUNK else None
        if what == "merge":
            return self._merge() if big else None
        if what == "icp":
            rec = self._query("nearest", "icp", outputs="both") if big else None
            if rec is not None:
                # (the radius reaches what the move displaces: the second query is to find the moved points)
                g = given_points(rec, mo).astype(np.float64)
                g = g[np.isfinite(g).all(axis=1)]
                M = em.MATRICES["rigid"]
                with np.errstate(all="ignore"):
                    shift = np.median(np.linalg.norm(g @ M[:3, :3].T + M[:3, 3] - g, axis=1)) if len(g) else 0.0
                    r = f32(1.0001 * (rec["radius"] + shift))
                if am._ok_radius(r):
                    rec["radius"] = float(r)
                self._then(("icp_move",), ("again", len(self.past), "icp_again"))
            return rec
        if what == "copies":
            rec = self._copies("append_copies") if big else None
            if rec is not None:
                self._then(("ties", "nearest_k", "copies"), ("remove_originals", rec, mo.n), ("ties", None, "survivors"))
            return rec
        if what == "sorted":
            if not big:
                return None
            if not mo.sorted:
                self._then(("sorted",))
                return {"call": "reorder", "edge": None}
            rec = self._copies("append_copies_sorted")
            if rec is not None:
                self._then(("ties", QUERIES[self.seed % 2], "copies"), ("reorder",), ("again", len(self.past) + 1, "reordered"))
            return rec
        e = item[1]
        if e == "directed_write":
            if mo.n < 2 * em.CHUNK:
                return None
            if mo.keep is None:
                self._then(item)
                return self._keep(("random", self._seed(), 0.8))
            rec = self._write(("range", 3, em.CHUNK + 9), 0.0, 1.0, ("both", "xyz")[self.seed % 2])
            rec["edge"] = "directed_write"
            self._then(("query",))
            return rec
        if e == "remove_all_then_append":
            self._then(("append_empty",), ("query",))
            return self._remove(("none",), e)
        if not big and not e.startswith("append"):
            return None
        rec = self._edge(e)
        self.forced = []  # (edit_model's own followers have no room here)
        if rec is None and e.startswith("move_"):
            # (no random range of the front half may move so: the longest run of points that may, if it has 8 or more)
            ok = (self.level <= 0) if e == "move_scale_shear" else (self.level >= 0) & ~self.thrown
            run = np.concatenate([[0], ok[:max(1, mo.n // 2)].astype(np.int8), [0]])
            a, b = np.flatnonzero(np.diff(run) == 1), np.flatnonzero(np.diff(run) == -1)
            if a.size and (b - a).max() >= 8:
                j = int(np.argmax(b - a))
                rec = self._move(e[5:], ("range", int(a[j]), int(b[j])), e)
        if rec is not None:  # (behind a move the k nearest, the nearest in the ICP step that follows)
            self._then(("query", "nearest_k") if e.startswith("move_") else ("query",))
        return rec

    def _then(self, *items):
        self.queue[:0] = items

    def _continue(self, item):
        mo, what = self.model, item[0]
        if what == "query":
            return self._next_query(item[1:] or QUERIES)
        if what == "append_empty":
            return self._block("append", EMPTY_APPEND[self.seed % 3], "append_empty")
        if what == "icp_move":
            return self._move("rigid", None, "icp_move")
        if what == "again":  # (the record of step item[1] again; "ref": that step's very arrays)
            rec = dict(self.recs[item[1]], edge=item[2], state=self._qstate())
            if item[2] == "icp_again":
                rec["given"] = {"ref": item[1]}
            return rec
        if what == "ties":
            src = self.past[-1]["src"] if "src" in self.past[-1] else None
            if item[2] == "copies":
                lo, hi = mo.n - src.size, mo.n
            else:  # (what is left of the triples: the first of their two copies)
                lo, hi = mo.n - self.left[0], mo.n - self.left[0] + self.left[1]
            kind = item[1] or QUERIES[(self.seed + 1) % 2]
            return self._query(kind, item[2], ties=(lo, hi), k=(2, 8)[self.seed % 2] if kind == "nearest_k" else None)
        if what == "remove_originals":
            src, base = item[1], item[2]
            self.left = (src["count"] + src["count"] // 3, src["count"] // 3)
            return {"call": "remove_originals", "seed": src["seed"], "count": src["count"], "base": base, "form": self._form(),
                    "edge": "remove_originals"}
        if what == "reorder":
            return {"call": "reorder", "edge": "reorder"}
        return self._start(item)

    def _random(self):
        if self.model.n > 0 and self.qrng.random() < 0.34:
            rec = self._next_query(NEW if self.i < STEPS - 1 else QUERIES)  # (a merge has a query behind it: not last)
            if rec is not None:
                return rec
        return wm._Gen._random(self)  # (write_model's steps: the six older analysis kinds have their own sequences)

    # -- what the last edit touched
    def _note(self, rec, args, before):
        mo, call = self.model, rec["call"]
        if call in ("query",):
            self.prev = (rec["kind"], rec["edge"])
            self.follow = False
            return
        if call in ("merge", "append_copies"):
            hot = np.asarray(args["G"][self.done_new] if call == "merge" else args["xyz"], np.float64).reshape(-1, 3)
            hot = hot[np.isfinite(hot).all(axis=1)]
            if mo.n > before.n:
                self.hot = hot if len(hot) else None
                self.touched = np.arange(mo.n) >= before.n
            self.prev, self.follow = (call, rec["edge"]), False
            return
        super()._note(dict(rec, call="remove") if call == "remove_originals" else rec, args, before)
        self.prev = (call, rec["edge"])
        self.follow = False  # (the chains bring their own queries)

    def _track(self, rec, args, n0):
        call = rec["call"]
        if call in ("merge", "append_copies"):
            m = self.model.n - n0
            self.level = np.concatenate([self.level, np.zeros(m, np.int8)])
            self.thrown = np.concatenate([self.thrown, np.zeros(m, bool)])
        elif call == "remove_originals":
            self.level, self.thrown = self.level[args["bits"]], self.thrown[args["bits"]]
        elif call != "query":
            super()._track(rec, args, n0)

    def step(self, i):
        """A chain in progress goes on; else upkeep (a cloud of three chunks or fewer grows); else the next chain of the
        agenda starts, at every other step or when the steps left are no more than the agenda needs; else a random
        step, a third of them queries and merges."""
        rec, mo, self.i = None, self.model, i
        if i == 0:
            rec = self._block("upload", int(self.rng.choice(em.START_COUNTS)))
        while rec is None and self.queue:
            rec = self._continue(self.queue.pop(0))
        if rec is None and 0 < mo.n <= 3 * em.CHUNK and self.prev[0] == "upload":  # (a small start cloud is queried)
            rec = self._next_query()
        if rec is None and mo.n <= 3 * em.CHUNK:
            rec = self._block("append", int(self.arng.integers(3 * em.CHUNK + 1, 3000)))
        if rec is None and self.agenda:
            need = 1 + sum({"span": 1, "selected": 8, "copies": 4, "sorted": 5, "edge": 3}[a[0]] for a in self.agenda)
            if i % 2 == 0 or STEPS - i <= need:
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
        if rec["call"] == "merge":
            self.done_new = res["new"]
        self._track(rec, args, n0)
        self._note(rec, args, before)
        assert mo.n <= em.N_MAX and self.level.shape == self.thrown.shape == (mo.n,)
        self.past.append(args)
        self.recs.append(rec)
        self.done = (rec, args, res, n0, before.selection, None if mo.selection is None else mo.selection.copy())
        return rec


@functools.lru_cache(maxsize=None)
def replay(seed, family, steps=STEPS):
    """[(record, arguments, result, n before, selection before, selection after)] of the sequence on the model alone, a
    pure function of the arguments (result: None for a step that is neither query nor merge).  The references are
    computed once, while the sequence is drawn, and shared by every test that needs them: cached, read, never changed."""
    g, out = _Gen(int(seed), family), []
    for i in range(steps):
        g.step(i)
        out.append(g.done)
    return tuple(out)


def sequence(seed, family, steps=STEPS):
    """`steps` step records: write_model.sequence's calls with queries, merges and their directed edits among them."""
    return tuple(r[0] for r in replay(seed, family, steps))


def frame_steps(steps):
    return em.frame_steps(steps)


# Regressions: prefixes of random sequences that failed on the library, as literal steps: {name: (family, [records])}.
REGRESSIONS = {}
