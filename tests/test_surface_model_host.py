"""The checker and the inputs of test_gpu_surface_sequences.py, without a GPU, over exactly the seeds, families and step
count the GPU file runs: the five older generators' sequences are what they were (pinned digests); the model's
brute-force answers agree with the references' bucket forms, constant normals with plain clustering, the two facade
loops with the calls written out; the reference meets README_register.md's two conditions on every register step of
the sequences; every chain does what it is for; every call meets the states, the inputs and the directed edits the
device code branches on; trivial steps and the sensitivity to a stale cloud are measured against their caps
(tests/README_surface_sequences.md); and the GPU file's one comparison notices each way in which an answer could be
subtly wrong."""
import functools

import numpy as np

import analysis_model as am
import clusters_ref as cr
import edit_model as em
import nearest_k_ref
import nearest_model as nm
import nearest_ref
import register_ref as rr
import rows_model as rm
import segments_ref as sg
import select_ref
import surface_model as sm
import write_model as wm
from surface_model import CALLS, FAMILIES, KINDS, SEEDS, STEPS
from test_analysis_model_host import EDIT_DIGEST, WRITE_DIGEST, _digest
from test_nearest_model_host import ANALYSIS_DIGEST, NEAREST_DIGEST, _renumber, _through
from test_register_host import ANGLE_PLANE, ANGLE_POINT, MARGIN, ORTHO_PLANE, ORTHO_POINT
from test_rows_model_host import ROWS_DIGEST

CASES = [(family, seed) for family in sorted(FAMILIES) for seed in SEEDS]
f32, f64 = np.float32, np.float64
NONE = nearest_ref.NONE
REGISTERS = ("register", "register_loop")
REMOVERS = ("remove", "remove_originals")
APPENDS = ("append", "append_copies", "append_near", "append_mirrors")


def _steps(family=None):
    """(family, seed, step index, record, arguments, result, n before) of every surface step of the named sequences."""
    for fam, sd in CASES:
        if family is None or fam == family:
            for i, (rec, args, res, n0, s0, s1) in enumerate(sm.replay(sd, fam)):
                if rec["call"] == "surface":
                    yield fam, sd, i, rec, args, res, n0


def _good(family=None, kind=None):
    return [s for s in _steps(family) if s[5]["error"] is None and (kind is None or s[3]["kind"] == kind)]


@functools.lru_cache(maxsize=None)
def _states(family, seed):
    """The model before every step of a sequence, and after the last (a surface or rows step through its cached result)."""
    model, out = sm.Model(family), []
    for rec, args, res, n0, s0, s1 in sm.replay(seed, family):
        out.append(model.copy())
        if rec["call"] in ("surface", "rows"):
            sm.advance(model, rec, res)
        else:
            sm.apply(model, rec, args)
    return out + [model.copy()]


def _full(rec):
    """The record with every output asked for: the comparisons below are about values, not about placement."""
    if rec["kind"] == "segments":
        return dict(rec, labels="host", stats=True)
    return dict(rec, ask=list(sm.ASKS[0])) if rec["kind"] == "register" else rec


def _on(state, rec, args, **change):
    """The record's answer on another state of the cloud: the inputs its source names there, the given points as they are."""
    a = dict(args)
    if rec["kind"] == "segments" or rec.get("plane"):
        a["normals"], a["curvature"] = state.inputs(rec)
    a.update(change)
    return sm.apply(state.copy(), rec, a)


def _kept_bits(rec, args, res):
    """The keep bits of a step that removes points (None: it is none)."""
    if rec["call"] in REMOVERS:
        return args["bits"]
    if rec["call"] == "rows" and rec["kind"] == "cleanup" and res["error"] is None:
        return res["hit"]
    if rec["call"] == "surface" and rec["kind"] == "remove_small_segments" and res["error"] is None:
        return res["hit"]
    return None


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_the_older_sequences_are_unchanged():
    assert _digest(em, em.FAMILIES) == EDIT_DIGEST
    assert _digest(wm, wm.WRITE_FAMILIES) == WRITE_DIGEST
    assert _digest(am, am.FAMILIES) == ANALYSIS_DIGEST
    assert _digest(nm, nm.FAMILIES) == NEAREST_DIGEST
    assert _digest(rm, rm.FAMILIES) == ROWS_DIGEST
    assert (rm.SEEDS, rm.STEPS, nm.STEPS, am.STEPS) == (SEEDS, STEPS, STEPS, STEPS) and set(rm.FAMILIES) == set(FAMILIES)


def test_sequences_are_a_pure_function_of_their_arguments():
    for family, seed in CASES:
        a = sm.sequence(seed, family, STEPS)
        assert len(a) == STEPS and a[0]["call"] == "upload", (family, seed)
        if (seed, family) == (SEEDS[0], "specials"):  # (drawn again, past the cache)
            assert a == tuple(r[0] for r in sm._replay.__wrapped__(seed, family, STEPS)), (family, seed)
        assert sm.sequence(seed, family, 10) == a[:10], (family, seed)  # (a prefix reproduces a failure)
    assert (SEEDS, STEPS) == ((1, 2, 3), 30) and set(FAMILIES) == set(em.FAMILIES) and len(CASES) == 18 and sm.REGRESSIONS == {}


def test_records_say_where_they_stand():
    for family, seed in CASES:
        recs, states = sm.sequence(seed, family), _states(family, seed)
        for i, rec in enumerate(recs):
            assert states[i].n <= em.N_MAX
            if rec["call"] == "surface":
                prev = recs[i - 1]
                assert rec["state"]["after"] == (prev["kind"] if prev["call"] in ("surface", "rows") else prev["call"]), (family, seed, i)
                assert rec["state"]["after_edge"] == prev["edge"], (family, seed, i)
                assert rec["state"]["n"] == states[i].n and rec["state"]["sorted"] == states[i].sorted, (family, seed, i)
            if rec["edge"] in sm.SHARED + ("append_empty",) and rec["edge"] != "remove_all_then_append":  # (its append comes first)
                assert [r["call"] for r in recs[i + 1:i + 3]] == ["surface", "surface"], (family, seed, i)
                assert {r["kind"] for r in recs[i + 1:i + 3]} == set(CALLS), (family, seed, i)


# ---- the model against the definitions -------------------------------------------------------------------------------------
def test_brute_agrees_with_the_bucket_forms():
    seg = reg = refused = 0
    for fam, sd, i, rec, args, res, n0 in _good():
        st, kind = _states(fam, sd)[i], rec["kind"]
        if kind == "segments":
            lim = rec["max_curvature"]
            curv, lim = (None, np.inf) if lim is None else (args["curvature"], lim)
            brute = sg.labels_brute(st.xyz, rec["radius"], rec["cos_angle"], args["normals"], curv, lim, rec["oriented"])
            assert np.array_equal(brute, res["labels"]), (fam, sd, i)
            try:
                edges = sg.edges(st.xyz, rec["radius"], rec["cos_angle"], args["normals"], curv, lim, rec["oriented"])
            except ValueError:  # (the bucket forms' own grid, anchored elsewhere, ends a little before the library's span does)
                assert rec["edge"] == "at_span", (fam, sd, i)
                refused += 1
                continue
            assert np.array_equal(brute, cr.labels_of_pairs(st.n, *edges)), (fam, sd, i)
            seg += 1
        elif kind == "register":
            try:
                other = st.register(args["G"], rec["radius"], rec["plane"], args["pose"], args.get("normals"), finder=nearest_ref.nearest_bucket)
            except ValueError:
                assert rec["edge"] == "at_span", (fam, sd, i)
                refused += 1
                continue
            assert sm.mismatches(sm.outputs(_full(rec), other), sm.outputs(_full(rec), res)) == [], (fam, sd, i)
            reg += 1
    assert seg >= 120 and reg >= 120 and refused <= 18, (seg, reg, refused)


def test_constant_normals_are_plain_clustering():
    seen = 0
    for fam, sd, i, rec, args, res, n0 in _good(kind="segments"):
        if rec["source"] == "constant":
            assert rec["max_curvature"] is None and args["curvature"] is None
            assert np.array_equal(res["labels"], cr.labels(_states(fam, sd)[i].xyz, rec["radius"])), (fam, sd, i)
            seen += 1
    assert seen >= 6, seen


def test_the_facade_loops_are_the_calls_written_out():
    loops = removals = 0
    for family, seed in CASES:
        rp, states = sm.replay(seed, family), _states(family, seed)
        for i, (rec, args, res, n0, s0, s1) in enumerate(rp):
            if rec["call"] != "surface" or res["error"] is not None:
                continue
            before, after = states[i], states[i + 1]
            if rec["kind"] == "register_loop":  # (ProjectCloud.registerPoints, step by step through Model.register)
                cur, rms, prev = list(rr.IDENTITY) if args["pose"] is None else [float(v) for v in args["pose"]], [], None
                for _ in range(rec["iterations"]):
                    one = before.register(args["G"], rec["radius"], rec["plane"], cur, args.get("normals"))
                    rms.append(rr.rms_of(one["moments"], rec["plane"]))
                    if one["stats"][3] or (prev is not None and one["stats"][0] == prev[0] and not rms[-1] < prev[1]):
                        break
                    prev = (one["stats"][0], rms[-1])
                    cur = rr.compose(one["step"], cur)
                assert rms == res["rms"] and np.array_equal(rr.bits64(np.array(cur)), rr.bits64(res["pose"][:3]).reshape(-1)), (family, seed, i)
                assert after.n == before.n and (s0 is None) == (s1 is None)
                loops += 1
            if rec["kind"] == "remove_small_segments":
                e = before.normals(rec["k"], rec["radius"])
                lab = sg.labels(before.xyz, rec["radius"], f32(np.cos(rec["angle"])), e["normals"], e["curvature"], rec["max_curvature"])
                hit = sg.hits(lab, rec["min_points"])
                assert np.array_equal(hit, res["hit"]) and res["removed"] == int((~hit).sum()), (family, seed, i)
                want = em.Model(family)
                want.__dict__.update(em.Model.copy(before).__dict__)
                want.remove(hit)
                assert np.array_equal(after.xyz.view(np.uint32), want.xyz.view(np.uint32)) and np.array_equal(after.rgb, want.rgb)
                assert after.selection is None and (after.keep is None) == (want.keep is None), (family, seed, i)
                removals += 1
    assert loops >= 12 and removals >= 18, (loops, removals)


def test_span_steps_sit_where_they_say():
    for fam, sd, i, rec, args, res, n0 in _steps():
        if rec["edge"] not in sm.SPAN:
            continue
        before, after = _states(fam, sd)[i], _states(fam, sd)[i + 1]
        xyz = before.xyz
        if rec["edge"] == "pose_span":  # (the pose alone carries a point out: the given points themselves lie inside)
            G = args["G"]
            assert not sm.beyond_span(G, rec["radius"]).any() and sm.beyond_span(rr.posed(G, args["pose"]), rec["radius"]).any()
            assert res["error"] == "unsupported" and not sm.beyond_span(xyz, rec["radius"]).any(), (fam, sd, i)
        elif rec["edge"] == "beyond_span":
            assert sm.beyond_span(xyz, rec["radius"]).any() and res["error"] == "unsupported", (fam, sd, i)
        else:
            fin = xyz[np.isfinite(xyz).all(axis=1)]
            assert not sm.beyond_span(xyz, rec["radius"]).any() and res["error"] is None, (fam, sd, i)
            q = np.abs(np.floor(fin.astype(f64) / am.cell_edge(rec["radius"])))
            assert q.max() >= 0.98 * 2 ** 20, (fam, sd, i)  # (the outermost points lie in the last cells)
        if res["error"] is not None:  # (nothing moved)
            assert after.n == before.n and np.array_equal(after.xyz.view(np.uint32), xyz.view(np.uint32))
            assert (after.selection is None) == (before.selection is None)
            assert after.selection is None or np.array_equal(after.selection, before.selection)


def test_the_reference_meets_its_two_conditions_on_every_register_step():
    """README_register.md's conditions, with test_register_host.py's bounds (names there: imported): the orthogonality
    defect of the step, and its angle against np.linalg.svd's Kabsch / np.linalg.solve's plane solution on the same
    pairs.  Conditions on the reference, no tolerance of the library."""
    worst = {"ortho_point": 0.0, "ortho_plane": 0.0, "angle_point": 0.0, "angle_plane": 0.0}
    seen = 0
    for fam, sd, i, rec, args, res, n0 in _good(kind="register"):
        if res["stats"][3]:
            continue
        mode = "plane" if rec["plane"] else "point"
        xyz = _states(fam, sd)[i].xyz
        with np.errstate(all="ignore"):
            P = rr.posed(args["G"], args["pose"])
            gi, used = rr.pairs(xyz, P, rec["radius"], args["normals"] if rec["plane"] else None, nearest_ref.nearest_brute)
        p, q = P[used].astype(f64), xyz[gi[used]].astype(f64)
        R = res["step"].reshape(3, 4)[:, :3]
        worst["ortho_" + mode] = max(worst["ortho_" + mode], float(np.abs(R.T @ R - np.eye(3)).max()))
        if rec["plane"]:
            om, tau, pb = rr.plane_solve(p, q, args["normals"][gi[used]].astype(f64))
            w = om / 2
            K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
            R2 = np.eye(3) + (2 / (1 + w @ w)) * (K + K @ K)
        else:
            R2, _ = rr.kabsch(p, q)
        angle = rr.rotation_angle(R, R2)
        worst["angle_" + mode] = max(worst["angle_" + mode], angle)
        seen += 1
    print("register steps", seen, "; " + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    assert seen >= 3 * len(CASES), seen  # (a sequence has three followed edits with a registration behind each, and its chains')
    assert worst["ortho_point"] <= MARGIN * ORTHO_POINT and worst["ortho_plane"] <= MARGIN * ORTHO_PLANE, worst
    assert worst["angle_point"] <= MARGIN * ANGLE_POINT and worst["angle_plane"] <= MARGIN * ANGLE_PLANE, worst


# ---- the chains ---------------------------------------------------------------------------------------------------------------
def _sans(rec):
    return {k: v for k, v in rec.items() if k not in ("edge", "state", "given")}


def _winners(state, rec, args):
    with np.errstate(all="ignore"):
        return nearest_ref.nearest_brute(state.xyz, rr.posed(args["G"], args["pose"]), rec["radius"])[0]


def test_the_chains_do_what_they_are_for():
    for family in sorted(FAMILIES):
        seen = {k: 0 for k in ("ties", "pipeline", "icp", "sorted", "seeded", "last_chunk", "degenerate", "emptied")}
        for sd in SEEDS:
            rp, states = sm.replay(sd, family), _states(family, sd)
            for i, (rec, args, res, n0, s0, s1) in enumerate(rp):
                edge, kind = rec["edge"], rec.get("kind")
                if edge == "append_empty":  # (700 given points on the 300, 37 or 255 of an emptied cloud: count > n)
                    reg = [r for r in rp[i + 1:i + 3] if r[0].get("kind") == "register"]
                    assert len(reg) == 1 and reg[0][2]["error"] is None and len(reg[0][1]["G"]) == 700 > reg[0][3], (family, sd, i)
                    assert reg[0][3] in sm.EMPTY_APPEND and reg[0][2]["stats"][0] > reg[0][3]  # (more pairs than points: winners repeat)
                    seen["emptied"] += 1
                if rec["call"] != "surface":
                    continue
                if kind in REGISTERS:  # (no registration ever touches the selection)
                    assert (s0 is None) == (s1 is None) and (s0 is None or np.array_equal(s0, s1)), (family, sd, i)
                if edge == "ties_mirrors" and kind == "register":
                    a, b, c = rp[i - 6], rp[i - 3], rp[i]
                    assert [r[0]["call"] for r in rp[i - 8:i - 6]] == ["append_copies", "append_mirrors"]
                    assert (rp[i - 4][0]["call"], rp[i - 1][0]["edge"]) == ("remove_originals", "remove_copies")
                    assert a[0]["edge"] == "ties_originals" and b[0]["edge"] == "ties_copies" and a[1]["G"] is b[1]["G"] is c[1]["G"]
                    assert _sans(a[0]) == _sans(b[0]) and a[0]["plane"] and a[0]["source"] == "indexed" and not c[0]["plane"]
                    src = np.array(a[0]["given"]["indices"])
                    wa, wb, wc = (_winners(states[j], rp[j][0], rp[j][1]) for j in (i - 6, i - 3, i))
                    # the original wins at d2 = +0 ahead of its copy; then the copy, under its renumbered index and with
                    # another normal; then the smallest index of six mirrors at one distance
                    assert np.array_equal(wa, src) and not np.array_equal(wb, _through(wa, _renumber(rp[i - 4][1]["bits"])))
                    assert np.array_equal(states[i - 3].xyz[wb].view(np.uint32), a[1]["G"].view(np.uint32))
                    assert not np.array_equal(a[1]["normals"][wa], b[1]["normals"][wb])
                    assert not np.array_equal(rr.bits64(a[2]["moments"]), rr.bits64(b[2]["moments"])), (family, sd, i)
                    assert a[2]["stats"] == b[2]["stats"] == c[2]["stats"] == (src.size, 0, 0, 0), (family, sd, i)
                    k2 = nearest_k_ref.nearest_k_brute(states[i].xyz, c[1]["G"], rec["radius"], 6)
                    six = (k2[2] >= 6) & (k2[1][:, :6].view(np.uint32) == k2[1][:, :1].view(np.uint32)).all(axis=1)
                    assert six.sum() >= src.size // 2 and np.array_equal(wc[six], k2[0][six].min(axis=1)), (family, sd, i)
                    assert len(set(map(bytes, states[i].xyz[k2[0][six][0]].view(np.uint8)))) == 6  # (at different coordinates)
                    segs = [rp[j] for j in (i - 5, i - 2, i + 1)]
                    assert all(r[0]["kind"] == "segments" and r[0]["source"] == "indexed" and r[2]["error"] is None for r in segs)
                    assert _sans(segs[0][0]) == _sans(segs[1][0]) == _sans(segs[2][0])
                    seen["ties"] += 1
                if edge == "pipeline" and kind == "register":
                    chain = rp[i - 5:i + 1]
                    assert [(r[0]["call"], r[0].get("kind")) for r in chain] == [("rows", "normals"), ("surface", "segments"),
                            ("surface", "remove_small_segments"), ("rows", "normals"), ("surface", "segments"), ("surface", "register")]
                    n1, s1_, rem, n2, s2_, reg = chain
                    assert all(r[2]["error"] is None for r in chain), (family, sd, i)
                    assert s1_[0]["held"] and s2_[0]["held"] and reg[0]["held"] and reg[0]["plane"] and s1_[0]["op"] == "replace"
                    assert s1_[0]["max_curvature"] is not None and _sans(s1_[0]) == _sans(s2_[0])
                    assert s1_[1]["normals"] is n1[2]["normals"] or np.array_equal(s1_[1]["normals"].view(np.uint32), n1[2]["normals"].view(np.uint32))
                    assert np.array_equal(reg[1]["normals"].view(np.uint32), n2[2]["normals"].view(np.uint32))
                    assert np.array_equal(rem[2]["hit"], s1_[2]["hit"]) and rem[3] - rem[2]["removed"] == n2[3] == reg[3]
                    seen["pipeline"] += 1
                if edge == "icp_again":
                    a, mv = rp[i - 2], rp[i - 1]
                    assert a[0]["edge"] == "icp" and mv[0]["edge"] == "icp_move" and a[1]["G"] is args["G"] and _sans(a[0]) == _sans(rec)
                    assert rec["iterations"] <= 6 and a[0]["pose"] is not None
                    assert a[2]["error"] is None and res["error"] is None and sm.mismatches(sm.outputs(rec, res), sm.outputs(rec, a[2]))
                    seen["icp"] += 1
                if edge == "reordered":
                    j = i - 3
                    assert rp[j][0]["edge"] == "sorted" and rp[j][0]["kind"] == kind and _sans(rp[j][0]) == _sans(rec), (family, sd, i)
                    assert states[j].sorted and [r[0]["call"] for r in rp[j + 1:i] if r[0]["call"] != "surface"] == ["reorder"]
                    assert sm.mismatches(sm.outputs(_full(rec), res), sm.outputs(_full(rec), rp[j][2])) == [], (family, sd, i)
                    seen["sorted"] += kind == "segments"
                if edge == "seeded":
                    if kind == "segments":
                        assert rp[i - 1][0]["call"] == "select" and s0 is not None and rec["seeded"]
                        assert (rec["op"], rec["outside"], rec["oriented"]) == sm.SEEDED[sorted(FAMILIES).index(family)], (family, sd, i)
                        assert rp[i + 1][0]["kind"] == "register" and rp[i + 2][0]["call"] == "transform", (family, sd, i)
                        again = rp[i + 3]
                        assert again[0]["edge"] == "seeded_again" and _sans(again[0]) == _sans(rec) and again[4] is not None
                        seen["seeded"] += 1
                    else:
                        assert s0 is not None and np.array_equal(s0, s1), (family, sd, i)
                if edge == "last_chunk_only":
                    w = _winners(states[i], rec, args)
                    assert n0 % em.CHUNK and (w[w != NONE] >= em.CHUNK * (n0 // em.CHUNK)).all() and (w != NONE).sum() >= 8, (family, sd, i)
                    nxt, far = rp[i + 1], rp[i + 2]
                    w = _winners(states[i + 1], nxt[0], nxt[1])
                    assert nxt[0]["edge"] == "first_chunk_only" and (w[w != NONE] < em.CHUNK).all() and (w != NONE).sum() >= 8
                    assert far[0]["edge"] == "no_pair" and far[2]["stats"][0] == 0 and far[2]["stats"][1] == 64 and far[2]["stats"][3] == 1
                    assert not far[2]["moments"].any() and np.array_equal(far[2]["step"], np.array(rr.IDENTITY))
                    seen["last_chunk"] += 1
                if edge == "degenerate_plane":
                    two = rp[i + 1]
                    assert rec["plane"] and rec["source"] == "constant" and res["stats"][3] == 1 and res["stats"][0] >= 6, (family, sd, i)
                    assert two[0]["edge"] == "degenerate_point" and two[2]["stats"][0] == 2 and two[2]["stats"][3] == 1
                    for r in (res, two[2]):  # (the identity step, the moments there all the same)
                        assert np.array_equal(r["step"], np.array(rr.IDENTITY)) and r["moments"][0] == r["stats"][0]
                    seen["degenerate"] += 1
        assert all(v >= 1 for k, v in seen.items() if k != "sorted"), (family, seen)
        assert seen["sorted"] >= 1 or not em.allows_reorder(family), family


# ---- coverage -----------------------------------------------------------------------------------------------------------------
def test_coverage_in_every_family():
    missing = []  # (everything that is missing, at once)

    def need(ok, *what):
        if not ok:
            missing.append(what)

    emptied = set()
    for family in sorted(FAMILIES):
        steps = list(_steps(family))
        can_sort = em.allows_reorder(family) or FAMILIES[family].get("auto_reorder") == 1
        for kind in KINDS:
            good = _good(family, kind)
            need(len(good) >= 3, (family, kind, len(good)))
            states = [s[3]["state"] for s in good]
            need(any(st["chunks"] >= 3 for st in states), (family, kind, "three chunks"))
            need(any(st["mixed_scale"] for st in states), (family, kind, "mixed scale"))
            need(any(st["sorted"] for st in states) or not can_sort, (family, kind, "sorted"))
            if family == "specials":
                need(any(st["nonfinite"] for st in states), (family, kind, "non-finite"))
        behind = {k: set() for k in CALLS}
        for sd in SEEDS:
            rp = sm.replay(sd, family)
            for i, r in enumerate(rp):
                if r[0]["call"] != "surface" and r[0]["edge"] in sm.SHARED + ("append_empty",):
                    for nxt in rp[i + 1:i + 3]:
                        if nxt[0]["call"] == "surface" and nxt[0]["kind"] in CALLS:
                            behind[nxt[0]["kind"]].add(r[0]["edge"])
                if r[0]["edge"] == "append_empty":
                    emptied.add(r[0]["m"])
        for kind in CALLS:
            lack = set(sm.SHARED) - {"remove_all_then_append"} | {"append_empty"}
            need(behind[kind] >= lack, (family, kind, "behind every followed edit", sorted(lack - behind[kind])))
        reg = [s for s in _good(family, "register")]
        need({(s[3]["plane"], s[3]["pose"] is not None) for s in reg} == {(a, b) for a in (False, True) for b in (False, True)}, (family, "modes x pose"))
        need({len(s[4]["G"]) for s in reg} >= set(sm.GIVEN_ROTATION), (family, "given counts", sorted({len(s[4]["G"]) for s in reg})))
        need(any(len(s[4]["G"]) > s[6] for s in reg), (family, "count > n"))
        need({(s[3]["rows"], s[3]["width"]) for s in reg} == {(a, b) for a in ("host", "device") for b in (3, 4)}, (family, "rows x stride"))
        need({s[3]["where"] for s in reg if s[3]["plane"]} == {"host", "device"}, (family, "register normals host and device"))
        need({s[3]["source"] for s in reg if s[3]["plane"]} == set(sm.SOURCES), (family, "register sources"))
        need(any(s[5]["stats"][2] for s in reg) or family != "specials", (family, "a non-finite given point"))
        seg = [s for s in _good(family, "segments")]
        need({s[3]["source"] for s in seg} == set(sm.SOURCES), (family, "segments sources", sorted({s[3]["source"] for s in seg})))
        need({s[3]["where"] for s in seg} == {"host", "device"}, (family, "segments normals host and device"))
        need({s[3]["op"] for s in seg} == set(em.OPS), (family, "ops", sorted({s[3]["op"] for s in seg})))
        need({s[3]["outside"] for s in seg} == {False, True} and {s[3]["oriented"] for s in seg} == {False, True}, (family, "outside, oriented"))
        need({(s[3]["seeded"], s[3]["state"]["selection"]) for s in seg} >= {(True, True), (True, False), (False, False)}, (family, "seeded x selection"))
        lim = {s[3]["labels"] for s in seg if s[3]["max_curvature"] is not None}
        need(lim == set(sm.PLACES), (family, "a curvature limit with NULL, host and device labels", sorted(lim, key=str)))
        need(any(not s[3]["stats"] for s in seg) and any(s[3]["ask"] != list(sm.ASKS[0]) for s in reg), (family, "NULL stats"))
        edges = {(s[3]["kind"], s[3]["edge"]) for s in steps}
        for sd in SEEDS:
            mine = {(s[3]["kind"], s[3]["edge"]) for s in steps if s[1] == sd}
            need({("segments", "beyond_span"), ("segments", "at_span"), ("register", "pose_span")} <= mine, (family, sd, "span steps"))
        need(sum(s[3]["kind"] == "remove_small_segments" and s[3]["edge"] == "beyond_span" for s in steps) == 1, (family, "removal beyond_span"))
        need({("register", e) for e in ("degenerate_plane", "degenerate_point", "last_chunk_only", "first_chunk_only", "no_pair")} <= edges,
             (family, "directed register steps"))
    need(emptied == set(sm.EMPTY_APPEND), ("the appends behind a removal of every point", sorted(emptied)))
    # seeded steps on a LIVE selection (there, with a bit set), over all sequences: the six seeded chains among them
    live = [r[0] for c in CASES for r in sm.replay(c[1], c[0]) if r[0]["call"] == "surface" and r[0]["kind"] == "segments" and
            r[2]["error"] is None and r[0]["seeded"] and r[4] is not None and r[4].any()]
    need({r["op"] for r in live} >= set(sm.COMBINING), ("seeded on a live selection: ops", sorted({r["op"] for r in live})))
    for op in ("add", "toggle"):
        need({r["outside"] for r in live if r["op"] == op} == {False, True}, ("seeded on a live selection", op, "with and without outside"))
    need({r["outside"] for r in live} == {False, True} and {r["oriented"] for r in live} == {False, True}, "seeded on a live selection: outside, oriented")
    need({(r["op"], r["outside"], r["oriented"]) for r in live if r["edge"] == "seeded"} == set(sm.SEEDED), "the six seeded chains")
    every = list(_steps())
    for kind in CALLS:
        ns = {s[6] % 256 for s in every if s[3]["kind"] == kind and s[5]["error"] is None}
        need({0, 1, 255} <= ns, (kind, "n mod 256", sorted(ns)[:4], sorted(ns)[-2:]))
    need(any(s[3]["state"]["chunks"] == 1 for s in every), "a one-chunk cloud")
    need(max(s[6] for s in every) <= 4600, ("the largest cloud", max(s[6] for s in every)))
    assert missing == [], "\n".join(repr(m) for m in missing)


# ---- shares ----------------------------------------------------------------------------------------------------------------------
def _stale(rec, args, res, old, new, bits):
    """Does the step's answer on the cloud as it was BEFORE the previous edit (stale coordinates where the point count
    is unchanged, a stale point set otherwise) differ from `res`?  Labels and the partition through the survivors'
    indices, a registration through its moments."""
    was = _on(old, rec, args)
    if was["error"] != res["error"]:
        return True
    if res["error"] is not None:
        return False
    if rec["kind"] == "register":
        return not np.array_equal(rr.bits64(was["moments"]), rr.bits64(res["moments"]))
    a, b = was["labels"], res["labels"]
    if old.n == new.n:
        pass
    elif bits is not None:
        a = _through(a[bits], _renumber(bits))
    else:
        b = b[:old.n]
    return not np.array_equal(a, b)


def shares():
    """trivial steps / steps per kind (span steps and the directed trivial steps excluded, and counted on their own);
    stale-sensitive steps / steps of the two calls directly behind an edit of coordinates or the point set; the same
    behind a reorder."""
    triv = {k: [0, 0] for k in ("segments", "register", "remove_small_segments")}
    aside = {"span": 0, "directed": 0}
    for fam, sd, i, rec, args, res, n0 in _steps():
        if rec["edge"] in sm.SPAN or rec["edge"] in sm.DIRECTED_TRIVIAL:
            aside["span" if rec["edge"] in sm.SPAN else "directed"] += 1
            continue
        if res["error"] is not None:
            continue
        kind = "register" if rec["kind"] == "register_loop" else rec["kind"]
        triv[kind][1] += 1
        triv[kind][0] += sm.trivial(rec, res)
    stale, sort = [0, 0], [0, 0]
    for family, seed in CASES:
        states, rp = _states(family, seed), sm.replay(seed, family)
        for i in range(2, len(rp)):
            rec, args, res = rp[i][:3]
            prec, pargs, pres = rp[i - 1][:3]
            if rec["call"] != "surface" or rec["kind"] not in CALLS or rec["edge"] in sm.SPAN:
                continue
            old, new = states[i - 1], states[i]
            bits = _kept_bits(prec, pargs, pres)
            if prec["call"] == "reorder":
                sort[1] += 1
                sort[0] += _stale(rec, args, res, old, new, None)
                continue
            if old.n == new.n and np.array_equal(old.xyz.view(np.uint32), new.xyz.view(np.uint32)):
                continue
            if old.n == 0 or (old.n != new.n and bits is None and prec["call"] not in APPENDS):
                continue  # (behind an empty cloud or an upload of another size nothing can be laid side by side: not counted)
            stale[1] += 1
            stale[0] += _stale(rec, args, res, old, new, bits)
    return triv, aside, stale, sort


def test_shares_stay_within_their_caps():
    triv, aside, stale, sort = shares()
    for kind, (t, n) in triv.items():
        print("trivial", kind, t, "of", n)
        assert n >= 18 and 4 * t <= n, (kind, t, n)
    print("span steps", aside["span"], "; directed degenerate and no-pair steps", aside["directed"])
    print("stale-sensitive", stale[0], "of", stale[1], "; behind a reorder", sort[0], "of", sort[1])
    assert stale[1] >= 60 and 2 * stale[0] >= stale[1], stale
    assert sort[0] == 0 and sort[1] >= 4, sort  # (the model has no resident order; in every family that sorts)
    ns = [s[6] for s in _steps()]
    census = {k: sum(s[3]["kind"] == k for s in _steps()) for k in KINDS}
    print("points at the surface steps", min(ns), "..", int(np.median(ns)), "..", max(ns), "; surface steps", len(ns), census)


# ---- the comparison can fail ----------------------------------------------------------------------------------------------------
def _largest_labels(lab):
    top = np.zeros(lab.size, np.uint32)
    np.maximum.at(top, lab, np.arange(lab.size, dtype=np.uint32))
    return top[lab]


def _resident_order(xyz):
    """A stand-in for the order a sort leaves the points in (the model has none): by x, then y, then z."""
    return np.lexsort((xyz[:, 2], xyz[:, 1], xyz[:, 0]))


def _larger_tie(A, P, radius):
    """nearest_ref.nearest_brute with every tie in d2 bits resolved to the LARGER of the first two indices."""
    gi = nearest_ref.nearest_brute(A, P, radius)[0].copy()
    idx, d2, found, _ = nearest_k_ref.nearest_k_brute(A, P, radius, 2)
    tied = (found >= 2) & (d2[:, 0].view(np.uint32) == d2[:, 1].view(np.uint32))
    gi[tied] = idx[tied, 1]
    return (gi,)


def _without_last_chunk(A, P, radius):
    gi = nearest_ref.nearest_brute(A, P, radius)[0].copy()
    n = np.asarray(A).shape[0]
    gi[(gi != NONE) & (gi >= em.CHUNK * ((n - 1) // em.CHUNK))] = NONE
    return (gi,)


def _edit_before(rp, i):
    """The last step before step i that may have changed the cloud: the steps of the two calls between leave it alone."""
    j = i - 1
    while j > 0 and rp[j][0]["call"] == "surface" and rp[j][0]["kind"] != "remove_small_segments":
        j -= 1
    return j


def test_the_comparison_notices_each_kind_of_wrong_answer():
    names = ("renumber", "slot", "largest", "gather", "chunk_segments", "chunk_register", "old_normal", "tie", "last_chunk", "tail", "fold")
    for family in sorted(FAMILIES):
        seen = dict.fromkeys(names, 0)
        for fam, sd, i, rec, args, res, n0 in _good(family):
            if rec["kind"] not in CALLS or all(seen.values()):
                continue
            rec = _full(rec)
            rp, states = sm.replay(sd, fam), _states(fam, sd)
            st, true = states[i], sm.outputs(rec, res)
            assert sm.mismatches(true, sm.outputs(rec, res)) == []
            j = _edit_before(rp, i)
            prec, pargs, pres = rp[j][:3]
            bits = _kept_bits(prec, pargs, pres)
            removal = bits is not None and not bits.all() and bits.any()
            moved = prec["call"] == "transform"
            if moved:
                idx = np.flatnonzero(np.ones(n0, bool) if pargs["bits"] is None else pargs["bits"])
                stale = []
                for c in np.unique(idx // em.CHUNK)[:3]:  # (one 256-point chunk with its coordinates from before the move)
                    m = st.copy()
                    m.xyz[c * em.CHUNK:(c + 1) * em.CHUNK] = states[j].xyz[c * em.CHUNK:(c + 1) * em.CHUNK]
                    stale.append(m)
            if rec["kind"] == "segments":
                lab = res["labels"]
                if removal and not seen["renumber"]:  # (the labels of before the removal, under the survivors' OLD indices)
                    was = _on(states[j], rec, args)
                    if was["error"] is None:
                        seen["renumber"] += "labels" in sm.mismatches(dict(true, labels=was["labels"][bits]), true)
                if not seen["slot"] and n0 >= 3:
                    seen["slot"] += all(sm.mismatches(dict(true, labels=np.roll(lab, s)), true) == ["labels"] for s in (1, -1))
                if not seen["largest"] and res["stats"][1] < n0:
                    seen["largest"] += sm.mismatches(dict(true, labels=_largest_labels(lab)), true) == ["labels"]
                if st.sorted and not seen["gather"] and rec["source"] != "constant":
                    perm = _resident_order(st.xyz)
                    curv = args["curvature"]
                    alt = _on(st, rec, args)  # (the same inputs: nothing differs)
                    assert sm.mismatches(sm.outputs(rec, alt), true) == []
                    wrong = dict(args, normals=args["normals"][perm], curvature=None if curv is None else curv[perm])
                    seen["gather"] += bool(sm.mismatches(sm.outputs(rec, sm.apply(st.copy(), rec, wrong)), true))
                if moved and not seen["chunk_segments"]:
                    seen["chunk_segments"] += any(bool(sm.mismatches(sm.outputs(rec, _on(m, rec, args)), true)) for m in stale)
                if n0 % 64 and res["selection"][64 * (n0 // 64):].any() and not seen["tail"]:
                    sel = res["selection"].copy()
                    sel[64 * (n0 // 64):] = False
                    seen["tail"] += sm.mismatches(dict(true, selection=select_ref.words(sel)), true) == ["selection"]
                continue
            used = res["stats"][0]
            if moved and not seen["chunk_register"] and used:
                seen["chunk_register"] += any("moments" in sm.mismatches(sm.outputs(rec, _on(m, rec, args)), true) for m in stale)
            if removal and rec["plane"] and used and not seen["old_normal"]:
                # (the winner's normal read at the index it had BEFORE the removal)
                old = np.minimum(np.flatnonzero(bits), n0 - 1)
                alt = st.register(args["G"], rec["radius"], True, args["pose"], args["normals"][old])
                seen["old_normal"] += "moments" in sm.mismatches(sm.outputs(rec, alt), true)
            if rec["edge"] in ("ties_originals", "ties_copies", "ties_mirrors") and not seen["tie"]:
                alt = st.register(args["G"], rec["radius"], rec["plane"], args["pose"], args.get("normals"), finder=_larger_tie)
                seen["tie"] += "moments" in sm.mismatches(sm.outputs(rec, alt), true)
            if n0 % em.CHUNK and used and not seen["last_chunk"]:
                alt = st.register(args["G"], rec["radius"], rec["plane"], args["pose"], args.get("normals"), finder=_without_last_chunk)
                seen["last_chunk"] += alt["stats"][0] < used and {"moments", "stats"} <= set(sm.mismatches(sm.outputs(rec, alt), true))
            if used >= 300 and not res["stats"][3] and not seen["fold"]:
                # (two given points change places, so that two terms are added in other threads and waves of the fold --
                # the blocks hold 1024 given points and no step has more than 700: the sums differ in their last bits)
                G = args["G"].copy()
                G[[5, 300]] = G[[300, 5]]
                alt = st.register(G, rec["radius"], rec["plane"], args["pose"], args.get("normals"))
                a, b = alt["moments"], res["moments"]
                if alt["stats"] == res["stats"] and not np.array_equal(rr.bits64(a), rr.bits64(b)):
                    assert np.allclose(a, b, rtol=1e-9, atol=1e-9 * np.abs(b).max()), (fam, sd, i)
                    seen["fold"] += "moments" in sm.mismatches(sm.outputs(rec, alt), true)
        if not (em.allows_reorder(family) or FAMILIES[family].get("auto_reorder") == 1):
            seen["gather"] += 1  # (a family that never sorts has no permutation to gather through)
        assert all(v >= 1 for v in seen.values()), (family, sorted(k for k, v in seen.items() if not v))
