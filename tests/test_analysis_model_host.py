"""The checker and the inputs of test_gpu_analysis_sequences.py, without a GPU, over exactly the seeds, families and step
count the GPU file runs: edit_model's and write_model's own sequences are what they were (pinned digests); the span
transcription agrees with the references' cell helpers; every analysis kind meets the states the device code branches
on (three chunks or more, a chunk of mixed scales, a sorted cloud, non-finite points, selections made earlier, both span
edges); the steps are not trivial and are sensitive to a stale cloud (both measured, tests/README_analysis.md); and the
brute-force references the model uses agree with their bucket forms."""
import functools
import hashlib

import numpy as np

import analysis_model as am
import clusters_ref as cr
import edit_model as em
import near_ref
import neighbours_ref as nr
import voxel_ref
import write_model as wm
from analysis_model import FAMILIES, KINDS, SEEDS, STEPS

CASES = [(family, seed) for family in sorted(FAMILIES) for seed in SEEDS]
f32 = np.float32

# sha256 of repr() of every sequence of the two older generators, computed before analysis_model.py existed
EDIT_DIGEST = "323252e7f38737dcb44cc77fe57932c366491b15355aec34bb0eb843c6265ebc"
WRITE_DIGEST = "7087e43406afc739199b0a561cbbab0e9250cb0457b90a68c1a0d4f8d0d18ad5"


def _digest(mod, families):
    h = hashlib.sha256()
    for family in sorted(families):
        for seed in mod.SEEDS:
            h.update(repr((family, seed, list(mod.sequence(seed, family, mod.STEPS)))).encode())
    return h.hexdigest()


def _steps(family=None, seed=None):
    """(family, seed, step index, record, arguments, result, n before, selection before, selection after) of every
    analysis step of the named sequences."""
    for fam, sd in CASES:
        if (family is None or fam == family) and (seed is None or sd == seed):
            for i, (rec, args, res, n0, s0, s1) in enumerate(am.replay(sd, fam)):
                if rec["call"] == "analysis":
                    yield fam, sd, i, rec, args, res, n0, s0, s1


def test_the_older_sequences_are_unchanged():
    assert _digest(em, em.FAMILIES) == EDIT_DIGEST
    assert _digest(wm, wm.WRITE_FAMILIES) == WRITE_DIGEST


def test_sequences_are_a_pure_function_of_their_arguments():
    for family, seed in CASES:
        a = am.sequence(seed, family, STEPS)
        assert len(a) == STEPS and a[0]["call"] == "upload", (family, seed)
        if seed == SEEDS[0]:  # (drawn again, past the cache)
            assert a == tuple(r[0] for r in am.replay.__wrapped__(seed, family, STEPS)), (family, seed)
    assert am.sequence(SEEDS[0], "pack0", 12) == am.sequence(SEEDS[0], "pack0", STEPS)[:12]  # (a prefix reproduces a failure)
    assert set(FAMILIES) == set(em.FAMILIES)


def test_span_transcription():
    rng = np.random.default_rng(5)
    for r in (f32(0.013), f32(1.7), f32(2.0 ** -30)):
        h = am.cell_edge(r)
        assert h == float(r) * (1 + 2.0 ** -10)
        edge = np.array([am.CELL_MIN * h, (am.CELL_MAX + 1) * h], np.float64)
        p = np.concatenate([rng.uniform(-1.2, 1.2, 4000) * 2.0 ** 20 * float(r), edge, edge * (1 - 1e-6), edge * (1 + 1e-6),
                            [0.0, -0.0, np.inf, -np.inf, np.nan, 3.4e38, -3.4e38]]).astype(f32)
        got = am.axis_in_span(p, r)
        # the statement of include/rtr.h section 6h: -(2^20 - 1) h <= p < (2^20 - 1) h, decided on the quotient's floor
        for v, g in zip(p, got):
            want = bool(np.isfinite(v)) and am.CELL_MIN <= np.floor(float(v) / float(h)) <= am.CELL_MAX
            assert bool(g) == want, (r, v)
        inside = np.abs(p.astype(np.float64)) <= 2.0 ** 20 * float(r)
        assert got[inside & np.isfinite(p)].all()  # (every coordinate within +-2^20 radius has a cell)
        # near_ref's / neighbours_ref's foreign grid has cells twice as wide: a point in the span is far inside theirs
        # (where the few cells their BUCKET_ORIGIN shifts it by do not count)
        if r > 0.01:
            assert np.abs(near_ref._cells(np.stack([p, p, p], axis=1)[got], r)).max() < 2 ** 19 + 2 ** 10
        assert (am.beyond_span(np.stack([p, p, p], axis=1), r) == (np.isfinite(p) & ~got)).all()
    # a non-finite coordinate wins over an axis beyond the span: such a point is no error
    assert not am.beyond_span(f32([[np.nan, 1e30, 0.0]]), 1.0).any() and am.beyond_span(f32([[0, 1e30, 0.0]]), 1.0).all()


def test_span_steps_sit_where_they_say():
    model_of = {}
    for fam, sd, i, rec, args, res, n0, s0, s1 in _steps():
        if rec["edge"] is None:
            continue
        if (fam, sd) not in model_of:
            model_of[(fam, sd)] = _states(fam, sd)
        xyz = args["G"] if rec["kind"] == "near" else model_of[(fam, sd)][i].xyz
        fin = xyz[np.isfinite(xyz).all(axis=1)]
        far = am.beyond_span(xyz, rec["radius"])
        if rec["edge"] == "beyond_span":
            assert far.any() and res["error"] == "unsupported", (fam, sd, i)
        else:
            assert not far.any() and res["error"] is None and am.axis_in_span(fin, rec["radius"]).all(), (fam, sd, i)
            q = np.abs(np.floor(fin.astype(np.float64) / am.cell_edge(rec["radius"])))
            assert q.max() >= 0.98 * 2 ** 20, (fam, sd, i)  # (the outermost points lie in the last cells)


@functools.lru_cache(maxsize=None)
def _states(family, seed):
    """The model before every step of a sequence (an analysis step's effect, the selection, is replay's)."""
    model, out = am.Model(family), []
    for rec, args, res, n0, s0, s1 in am.replay(seed, family):
        out.append(model.copy())
        if rec["call"] == "analysis":
            model.selection = None if s1 is None else s1.copy()
        else:
            am.apply(model, rec, args)
    return out


def test_coverage_in_every_family():
    for family in sorted(FAMILIES):
        steps = list(_steps(family))
        can_sort = em.allows_reorder(family) or FAMILIES[family].get("auto_reorder") == 1
        for kind in KINDS:
            mine = [s for s in steps if s[3]["kind"] == kind]
            good = [s for s in mine if s[5]["error"] is None]
            assert len(good) >= 3, (family, kind, len(good))
            states = [s[3]["state"] for s in good]
            assert any(st["chunks"] >= 3 for st in states), (family, kind, "three chunks")
            assert any(st["mixed_scale"] for st in states), (family, kind, "mixed scale")
            assert any(st["sorted"] for st in states) or not can_sort, (family, kind, "sorted")
            assert not any(st["sorted"] for st in states) or can_sort, (family, kind)
            if family == "specials":
                assert any(st["nonfinite"] for st in states), (family, kind, "non-finite")
        seeded = [s[3]["state"]["selection"] for s in steps if s[3]["kind"] == "clusters" and s[3]["seeded"]
                  and s[5]["error"] is None]
        assert True in seeded and False in seeded, (family, "seeded clusters", seeded)
        for kind in ("bands", "fit_plane"):
            by = {s[3]["state"]["selection_by"] for s in steps if s[3]["kind"] == kind and s[3]["selected"]}
            assert by - {None}, (family, kind, "selected on a selection an earlier step made", by)
            assert {s[3]["selected"] for s in steps if s[3]["kind"] == kind} == {True, False}, (family, kind)
        for kind, edge in am.SPAN_STEPS:
            assert any(s[3]["kind"] == kind and s[3]["edge"] == edge for s in steps), (family, kind, edge)
        near = [s[3] for s in steps if s[3]["kind"] == "near"]
        assert {r["source"] for r in near} == {"host", "device"} and {r["width"] for r in near} == {3, 4}, family
        assert any(r["near"] for r in near) and any(r["given_only"] for r in near), family
        after = {s[3]["state"]["after_edge"] for s in steps}
        want = set(am.FOLLOWED) - (set() if em.allows_reorder(family) else {"reorder"})
        assert want <= after, (family, "edges an analysis step follows directly", sorted(want - after))
    ms = {s[3]["given"]["m"] for s in _steps() if s[3]["kind"] == "near"}
    assert ms == set(am.GIVEN_COUNTS), ms
    assert {len(s[3]["bands"]) for s in _steps() if s[3]["kind"] == "bands"} == {1, 64, 65}
    assert {s[3]["iterations"] for s in _steps() if s[3]["kind"] == "fit_plane"} == {16, 65}
    assert any(s[5]["error"] == "degenerate" for s in _steps() if s[3]["kind"] == "fit_plane")
    assert {(s[3]["min_points"], s[3]["max_points"]) for s in _steps() if s[3]["kind"] == "clusters"} == set(am.CLUSTER_WINDOWS)


def test_steps_are_directed_as_the_records_say():
    for family, seed in CASES:
        recs = am.sequence(seed, family, STEPS)
        for i, rec in enumerate(recs):
            if rec["call"] != "analysis":
                if i + 1 < len(recs) and rec["edge"] in am.FOLLOWED and am.replay(seed, family)[i + 1][3] >= 16:
                    assert recs[i + 1]["call"] == "analysis", (family, seed, i)  # (directly, where a cloud is there)
                continue
            prev = recs[i - 1]
            assert rec["state"]["after"] == (prev["kind"] if prev["call"] == "analysis" else prev["call"]), (family, seed, i)
            assert rec["state"]["after_edge"] == prev["edge"], (family, seed, i)
            assert rec["state"]["chunks"] <= em.N_MAX // em.CHUNK


def shares():
    """(trivial steps / steps per kind, span steps excluded; stale-sensitive steps / steps that follow an edit)."""
    triv = {k: [0, 0] for k in KINDS}
    for fam, sd, i, rec, args, res, n0, s0, s1 in _steps():
        if rec["edge"] is None and res["error"] is None:
            triv[rec["kind"]][1] += 1
            triv[rec["kind"]][0] += am.trivial(rec, res, n0)
    stale = [0, 0]
    for family, seed in CASES:
        states, rp = _states(family, seed), am.replay(seed, family)
        for i in range(2, len(rp)):
            rec, args, res = rp[i][:3]
            prec, pargs = rp[i - 1][:2]
            if rec["call"] != "analysis" or prec["call"] in ("analysis", "set_keep", "clear_keep", "select"):
                continue
            old, new = states[i - 1], states[i]
            moved = old.n != new.n or old.sorted != new.sorted or \
                not np.array_equal(old.xyz.view(np.uint32), new.xyz.view(np.uint32))
            if not moved:
                continue
            stale[1] += 1
            stale[0] += _differs(rec, args, res, prec, pargs, old, new)
    return triv, stale


def _partition_equal(a, b):
    return len(np.unique(a)) == len(np.unique(b)) == len(np.unique(np.stack([a, b], axis=1), axis=0))


def _differs(rec, args, res, prec, pargs, old, new):
    """Does the step's result on the cloud as it was BEFORE the previous edit (stale coordinates where the point count
    is unchanged, a stale point set otherwise, compared through the upload indices of the survivors) differ from `res`?"""
    if old.n == 0:
        return True
    m = old.copy()
    m.selection = None if new.selection is None or old.n != new.n else new.selection.copy()
    was = am.analyse(m, rec, args)
    if was["error"] != res["error"]:
        return True
    if res["error"] == "unsupported":
        return False
    if old.n == new.n:
        a = b = slice(None)  # (the same points, or an upload of as many: index by index)
    elif prec["call"] == "remove":
        a, b = pargs["bits"], slice(None)
    elif prec["call"] == "append":
        a, b = slice(None), slice(0, old.n)
    else:
        return True
    for key in ("hit", "labels", "near", "counts", "plane"):
        if res.get(key) is None:
            continue
        x, y = was[key], res[key]
        if key == "hit":
            x, y = x[a], y[b]
        if key == "labels":
            if not _partition_equal(x[a], y[b]):
                return True
        elif not np.array_equal(x, y):
            return True
    return False


def test_not_trivial_and_sensitive_to_a_stale_cloud():
    triv, stale = shares()
    for kind in KINDS:
        t, n = triv[kind]
        print("trivial", kind, t, "of", n)
        assert n >= 12 and 4 * t <= n, (kind, t, n)
    print("stale-sensitive", stale[0], "of", stale[1])
    assert stale[1] >= 100 and 2 * stale[0] >= stale[1], stale


def test_brute_references_agree_with_their_bucket_forms():
    done = 0
    for family, seed in (("pack2_ids", 1), ("sorted_blocks", 2), ("specials", 3)):
        model = max(_states(family, seed), key=lambda m: m.n)  # (the largest cloud of the sequence)
        fin = model.xyz[np.isfinite(model.xyz).all(axis=1)].astype(np.float64)
        assert model.n >= 256 and len(fin) >= 200, (family, seed, model.n)
        d = np.sqrt(((fin - fin[len(fin) // 2]) ** 2).sum(axis=1))
        for r in (f32(np.sort(d)[4]), f32(np.sort(d)[40])):
            if np.abs(fin).max() / (2.0 * float(r)) >= 2 ** 20 - 2:  # (the bucket forms refuse such a cloud)
                continue
            assert np.array_equal(nr.counts_bucket(model.xyz, r), nr.counts_brute(model.xyz, r)), (family, seed, r)
            assert np.array_equal(cr.labels(model.xyz, r), cr.labels_brute(model.xyz, r)), (family, seed, r)
            G = am.given_points({"given": {"m": 700, "radius": float(r), "data": 11, "box": 1, "at": None, "specials": 3}}, model)
            for x, y in zip(near_ref.near_bucket(model.xyz, G, r), near_ref.near_brute(model.xyz, G, r)):
                assert np.array_equal(x, y), (family, seed, r)
            h0, st0 = voxel_ref.select(model.xyz, 2 * r, fin[0], 2)
            h1, st1 = voxel_ref.select_loop(model.xyz, 2 * r, fin[0], 2)
            assert np.array_equal(h0, h1) and st0 == st1
            done += 1
    assert done >= 3
