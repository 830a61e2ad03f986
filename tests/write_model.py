"""edit_model.py with rtr_write_points in it (include/rtr.h section 2f): `Model` gains `write`, the sequences gain write
steps -- xyz / rgb / both, a random window of a random selection, host or device records -- among the appends, removals,
moves, masks, selections and sorts edit_model draws.  test_gpu_write_sequences.py drives the library with them,
test_write_host.py checks this file without a GPU.  numpy only.

A write record: "call" = "write"; "sel": None (every point) or a mask spec of edit_model.mask_bits; "form" as there;
"first" / "count": the window as fractions of the k selected points (count beyond the end is cut by the call);
"streams": "xyz", "rgb", "both" or "colour" (one broadcast colour); "source": "host" or "device"; "data" / "box": the
records (edit_model.block's generator); "state": what the cloud was when the step was drawn -- {"behind": points are
resident behind the last written chunk, "masked": a keep mask is in force, "sorted": the library has sorted it}."""
import numpy as np

import edit_model as em
import write_ref
from edit_model import FAMILIES, pose_for  # noqa: F401  (the GPU file's families and camera are edit_model's)

W, H = em.W, em.H
WRITE_FAMILIES = ("pack2_ids", "pack0", "sorted_blocks", "keep_soa")
SEEDS = (1, 2, 3)
STEPS = 24
STREAMS = ("xyz", "rgb", "both", "colour")


class Model(em.Model):
    def write(self, sel, first, X, C):
        """Record j of X (float32 rows) and / or C (uint8 rows, or one colour of shape (3,)) into the point of rank
        first + j of the selection (bool (n,), None = every point): write_ref.written on the model's arrays."""
        assert self.n > 0
        self.xyz, self.rgb, idx = write_ref.written(self.xyz, self.rgb, sel, first, X, C)
        if X is not None:
            self.loose[idx] = False  # (written coordinates are data again: bit for bit)
        return idx

    def copy(self):
        m = Model(self.family)
        base = em.Model.copy(self)
        m.__dict__.update(base.__dict__)
        return m


def window_of(rec, k):
    """(first, count) of a write record on a selection of k points."""
    first = int(rec["first"] * k)
    return first, int(np.ceil(rec["count"] * k))


def materialize(rec, model):
    if rec["call"] != "write":
        return em.materialize(rec, model)
    bits = None if rec["sel"] is None else em.mask_bits(rec["sel"], model)
    k = model.n if bits is None else int(bits.sum())
    first, count = window_of(rec, k)
    xyz, rgb = em.block({"m": count, "data": rec["data"], "box": rec["box"]})
    s = rec["streams"]
    return {"bits": bits, "first": first, "X": xyz if s in ("xyz", "both") else None,
            "C": rgb if s in ("rgb", "both") else (np.uint8(rgb[0]) if s == "colour" and count else
                                                  np.uint8([9, 8, 7]) if s == "colour" else None)}


def apply(model, rec, args):
    if rec["call"] != "write":
        return em.apply(model, rec, args)
    model.write(args["bits"], args["first"], args["X"], args["C"])


class _Gen(em._Gen):
    def __init__(self, seed, family):
        super().__init__(seed, family)
        self.model = Model(family)
        self.wrng = np.random.default_rng([seed, sorted(FAMILIES).index(family), 2])  # (the write steps' own chain)
        self.writes = 0
        self.write_due = False

    def _write(self, sel=None, first=None, count=None, streams=None, form=None):
        r, mo = self.wrng, self.model
        n = mo.n
        rec = {"call": "write", "sel": sel, "form": None if sel is None else (form or FORMS2[int(r.integers(2))]),
               "first": float(r.choice([0.0, 0.0, 0.25, 0.5, 0.9])) if first is None else first,
               "count": float(r.choice([1.0, 1.0, 0.5, 0.1, 0.01])) if count is None else count,
               "streams": streams or STREAMS[self.writes % len(STREAMS)], "source": ("host", "device")[self.writes % 2],
               "data": int(r.integers(1 << 30)), "box": int(r.integers(len(em.BOXES))), "edge": None}
        self.writes += 1
        bits = np.ones(n, bool) if sel is None else em.mask_bits(sel, mo)
        f, c = window_of(rec, int(bits.sum()))
        idx = np.flatnonzero(bits)[f:] if rec["streams"] == "colour" else np.flatnonzero(bits)[f:f + c]  # (one colour: to the end)
        last = (idx.max() // em.CHUNK + 1) * em.CHUNK if idx.size else n
        rec["state"] = {"behind": bool(idx.size and last < n), "masked": mo.keep is not None, "sorted": bool(mo.sorted),
                        "points": int(idx.size)}
        return rec

    def _random_write(self):
        mo, r = self.model, self.wrng
        if mo.selection is not None and r.random() < 0.5:
            return self._write(("selection",), form="device")
        u = r.random()
        if u < 0.25:
            return self._write(None)
        if u < 0.6:
            return self._write(("random", int(r.integers(1 << 30)), float(r.choice([0.05, 0.3, 0.7]))))
        a = int(r.integers(0, max(1, mo.n // 2)))  # (a range in the front half: points stay resident behind it)
        return self._write(("range", a, min(mo.n, a + int(r.integers(1, max(2, mo.n // 3))))), first=0.0, count=1.0)

    def _random(self):
        mo = self.model
        if mo.n > 0 and self.wrng.random() < 0.3:
            return self._random_write()
        return super()._random()

    def _track(self, rec, args, n0):
        if rec["call"] != "write":
            return super()._track(rec, args, n0)
        if args["X"] is not None:  # (the written points lie in a box of their own again)
            bits = np.ones(n0, bool) if args["bits"] is None else args["bits"]
            idx = np.flatnonzero(bits)[args["first"]:args["first"] + args["X"].shape[0]]
            self.level[idx], self.thrown[idx] = 0, False

    def step(self, i):
        """edit_model._Gen.step with three directed writes in front of it: once a cloud of two chunks or more is there,
        steps 7, 13 and 19 put a mask in force where there is none, from step 13 on sort the cloud where the family
        allows that (option point_ids), and write a range that ends in the second chunk -- behind a mask, in front of
        resident points, on a sorted cloud."""
        rec, mo = None, self.model
        if i == 0:
            rec = self._block("upload", int(self.rng.choice(em.START_COUNTS)))
        self.owed += i % 3 == 2
        if rec is None and not self.forced and mo.n >= 2 * em.CHUNK and (i in (7, 13, 19) or self.write_due):
            if mo.keep is None:
                rec, self.write_due = self._keep(("random", self._seed(), 0.8)), True
            elif i >= 13 and em.allows_reorder(self.family) and not mo.sorted:  # (the later ones on a sorted cloud)
                rec, self.write_due = {"call": "reorder", "edge": None}, True
            else:
                rec, self.write_due = self._write(("range", 3, em.CHUNK + 9), 0.0, 1.0, ("both", "xyz", "rgb")[i % 3]), False
        while rec is None and self.forced:
            rec = self._forced(self.forced.pop(0))
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
        args, n0 = materialize(rec, mo), mo.n
        apply(mo, rec, args)
        self._track(rec, args, n0)
        assert mo.n <= em.N_MAX and self.level.shape == self.thrown.shape == (mo.n,)
        return rec


FORMS2 = ("bool", "words")


def sequence(seed, family, steps):
    """`steps` step records, a pure function of the arguments: edit_model.sequence's calls with writes among them."""
    g = _Gen(int(seed), family)
    return [g.step(i) for i in range(steps)]


def frame_steps(steps):
    return em.frame_steps(steps)
