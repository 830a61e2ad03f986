"""The checker and the inputs of test_gpu_nearest_sequences.py, without a GPU, over exactly the seeds, families and step
count the GPU file runs: the three older generators' sequences are what they were (pinned digests); the model's
brute-force answers agree with the references' bucket forms, with each other and with the merge written out; every query
meets the states and the directed edits the device code branches on; ties, trivial steps, full and partly filled rows
and the sensitivity to a stale cloud are measured against their caps (tests/README_nearest_sequences.md); and the GPU
file's one comparison notices each way in which an answer could be subtly wrong."""
import functools

import numpy as np

import analysis_model as am
import edit_model as em
import near_ref
import nearest_k_ref
import nearest_model as nm
import nearest_ref
import write_model as wm
from nearest_model import FAMILIES, NONE, QUERIES, SEEDS, STEPS
from test_analysis_model_host import EDIT_DIGEST, WRITE_DIGEST, _digest

CASES = [(family, seed) for family in sorted(FAMILIES) for seed in SEEDS]
f32 = np.float32
# sha256 of repr() of every sequence of analysis_model, computed before nearest_model.py existed
ANALYSIS_DIGEST = "753ea2fb3699131760899274f5dfb509b992ef8f95a23e2f933d4a05fa073d29"
# the same of nearest_model's own sequences, computed when rows_model.py was written, before it touched anything
NEAREST_DIGEST = "a3a0032eac49aeaa8d4d109b069723b5b065ad33378edccbee7ece2fe3689838"
TIE_EDGES = ("copies", "survivors", "reordered")
REMOVALS = ("remove", "remove_originals")
APPENDS = ("append", "append_copies", "merge")


def _steps(family=None, call="query"):
    """(family, seed, step index, record, arguments, result, n before) of every step of `call` of the named sequences."""
    for fam, sd in CASES:
        if family is None or fam == family:
            for i, (rec, args, res, n0, s0, s1) in enumerate(nm.replay(sd, fam)):
                if rec["call"] == call:
                    yield fam, sd, i, rec, args, res, n0


def _good(family=None, kind=None):
    return [s for s in _steps(family) if s[5]["error"] is None and (kind is None or s[3]["kind"] == kind)]


@functools.lru_cache(maxsize=None)
def _states(family, seed):
    """The model before every step of a sequence, and after the last."""
    model, out = nm.Model(family), []
    for rec, args, res, n0, s0, s1 in nm.replay(seed, family):
        out.append(model.copy())
        if rec["call"] != "query":
            nm.apply(model, rec, args)
    return out + [model.copy()]


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_the_older_sequences_are_unchanged():
    assert _digest(em, em.FAMILIES) == EDIT_DIGEST
    assert _digest(wm, wm.WRITE_FAMILIES) == WRITE_DIGEST
    assert _digest(am, am.FAMILIES) == ANALYSIS_DIGEST
    assert _digest(nm, nm.FAMILIES) == NEAREST_DIGEST


def test_sequences_are_a_pure_function_of_their_arguments():
    for family, seed in CASES:
        a = nm.sequence(seed, family, STEPS)
        assert len(a) == STEPS and a[0]["call"] == "upload", (family, seed)
        if seed == SEEDS[0]:  # (drawn again, past the cache)
            assert a == tuple(r[0] for r in nm.replay.__wrapped__(seed, family, STEPS)), (family, seed)
        assert nm.sequence(seed, family, 12) == a[:12], (family, seed)  # (a prefix reproduces a failure)
    assert (SEEDS, STEPS) == ((1, 2, 3), 30) and set(FAMILIES) == set(em.FAMILIES) and len(CASES) == 18


def test_records_say_where_they_stand():
    for family, seed in CASES:
        recs, states = nm.sequence(seed, family), _states(family, seed)
        for i, rec in enumerate(recs):
            assert states[i].n <= em.N_MAX
            if rec["call"] in ("query", "merge"):
                prev = recs[i - 1]
                assert rec["state"]["after"] == (prev["kind"] if prev["call"] == "query" else prev["call"]), (family, seed, i)
                assert rec["state"]["after_edge"] == prev["edge"], (family, seed, i)
                assert rec["state"]["n"] == states[i].n and rec["given"].get("m", 0) <= 700, (family, seed, i)
                assert rec["state"]["sorted"] == states[i].sorted
            if rec["call"] == "merge" or rec["edge"] in nm.FOLLOWED + nm.DIRECTED:  # (a query directly behind it: none is last)
                assert i + 1 < len(recs) and recs[i + 1]["call"] == "query", (family, seed, i)


# ---- the model against the definitions -------------------------------------------------------------------------------------
def test_brute_answers_agree_with_the_bucket_forms_and_with_each_other():
    done = refused = 0
    for fam, sd, i, rec, args, res, n0 in _good():
        xyz, G, r = _states(fam, sd)[i].xyz, args["G"], rec["radius"]
        fin = G[np.isfinite(G).all(axis=1)]
        if rec["edge"] == "at_span" and np.abs(near_ref._cells(fin, r)).max() >= 2 ** 20:
            refused += 1  # (the bucket forms' own grid, anchored elsewhere, ends a little before the library's span does)
            continue
        near = near_ref.near_brute(xyz, G, r)[1]
        one = res["all"] if rec["kind"] == "nearest" else nearest_ref.nearest_brute(xyz, G, r)[:4]
        if rec["kind"] == "nearest":
            want = nearest_ref.nearest_bucket(xyz, G, r)
            assert nearest_ref.same(res["all"], want[:4]) and res["stats"] == want[4], (fam, sd, i)
            assert np.array_equal(res["all"][0] != NONE, near), (fam, sd, i)
        else:
            want = nearest_k_ref.nearest_k_bucket(xyz, G, r, rec["k"])
            assert nearest_k_ref.same((res["index"], res["dist2"], res["found"]), want[:3]) and res["stats"] == want[3], (fam, sd, i)
            assert np.array_equal(res["found"] > 0, near), (fam, sd, i)
            assert np.array_equal(res["index"][:, 0], one[0]), (fam, sd, i)
            assert np.array_equal(res["dist2"][:, 0].view(np.uint32), one[1].view(np.uint32)), (fam, sd, i)
        done += 1
    assert done >= 200 and refused <= 36, (done, refused)


def test_merge_is_append_where_the_near_bit_is_clear():
    done = 0
    for fam, sd, i, rec, args, res, n0 in _steps(call="merge"):
        before, after = _states(fam, sd)[i], _states(fam, sd)[i + 1]
        assert res["error"] is None, (fam, sd, i)
        a, g = before.xyz, args["G"]
        with np.errstate(all="ignore"):
            r2 = f32(rec["radius"]) * f32(rec["radius"])
            d = a[:, None, :] - g[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            near = ((d2 <= r2) & np.isfinite(a).all(axis=1)[:, None] & np.isfinite(g).all(axis=1)[None, :]).any(axis=0)
        assert np.array_equal(res["new"], ~near) and res["appended"] == int((~near).sum()), (fam, sd, i)
        assert not near[~np.isfinite(g).all(axis=1)].any()  # (a non-finite given point is new)
        assert np.array_equal(after.xyz.view(np.uint32), np.concatenate([a, g[~near]]).view(np.uint32)), (fam, sd, i)
        assert np.array_equal(after.rgb, np.concatenate([before.rgb, args["C"][~near]])), (fam, sd, i)
        if before.keep is not None:
            assert np.array_equal(after.keep, np.concatenate([before.keep, np.ones(res["appended"], bool)]))
        assert after.selection is None or res["appended"] == 0
        assert 4 * int(near.sum()) >= len(near), (fam, sd, i, "a quarter of the given points near resident ones")
        done += 1
    assert done >= 18, done


def test_span_steps_sit_where_they_say():
    for fam, sd, i, rec, args, res, n0 in _steps():
        if rec["edge"] not in ("beyond_span", "at_span"):
            continue
        G = args["G"]
        fin = G[np.isfinite(G).all(axis=1)]
        far = nm.beyond_span(G, rec["radius"])
        if rec["edge"] == "beyond_span":
            assert far.any() and res["error"] == "unsupported", (fam, sd, i)
        else:
            assert not far.any() and res["error"] is None and nm.axis_in_span(fin, rec["radius"]).all(), (fam, sd, i)
            q = np.abs(np.floor(fin.astype(np.float64) / am.cell_edge(rec["radius"])))
            assert q.max() >= 0.98 * 2 ** 20, (fam, sd, i)  # (the outermost points lie in the last cells)


# ---- coverage -----------------------------------------------------------------------------------------------------------------
def test_coverage_in_every_family():
    for family in sorted(FAMILIES):
        steps = list(_steps(family))
        can_sort = em.allows_reorder(family) or FAMILIES[family].get("auto_reorder") == 1
        for kind in QUERIES:
            good = _good(family, kind)
            assert len(good) >= 3, (family, kind, len(good))
            states = [s[3]["state"] for s in good]
            assert any(st["chunks"] >= 3 for st in states), (family, kind, "three chunks")
            assert any(st["mixed_scale"] for st in states), (family, kind, "mixed scale")
            assert any(st["sorted"] for st in states) or not can_sort, (family, kind, "sorted")
            assert not any(st["sorted"] for st in states) or can_sort, (family, kind)
            if family == "specials":
                assert any(st["nonfinite"] for st in states), (family, kind, "non-finite")
            for edge in ("beyond_span", "at_span"):  # (once in every sequence)
                assert sorted(s[1] for s in steps if s[3]["kind"] == kind and s[3]["edge"] == edge) == list(SEEDS), (family, kind, edge)
        after = {s[3]["state"]["after_edge"] for s in steps}
        want = set(nm.FOLLOWED) | set(nm.DIRECTED)
        if not em.allows_reorder(family):
            want -= {"reorder", "append_copies_sorted"}
        assert want <= after, (family, "edits a query follows directly", sorted(want - after))
        assert any(s[3]["state"]["after"] == "merge" for s in steps), family
        # (what follows is counted on the steps that succeed: a span step the host code refuses launches nothing)
        good = _good(family)
        assert {s[3]["k"] for s in good if s[3]["kind"] == "nearest_k"} == set(nm.KS), family
        near = [s[3] for s in good if s[3]["kind"] == "nearest"]
        assert {r["outputs"] for r in near if not r["match"]} == set(nm.OUTPUTS), family
        assert any(r["match"] for r in near), (family, "matchPoints")
        for kind in QUERIES:
            forms = {(s[3]["source"], s[3]["width"]) for s in good if s[3]["kind"] == kind}
            assert forms == {("host", 3), ("host", 4), ("device", 3), ("device", 4)}, (family, kind, forms)
            # a selection in force: the call leaves it alone, and the words compared behind it are some
            assert any(s[3]["state"]["selection"] for s in good if s[3]["kind"] == kind), (family, kind, "selection")
        merges = [(s[3]["state"]["selection"], s[5]["appended"]) for s in _steps(family, "merge") if s[5]["error"] is None]
        assert any(sel and app for sel, app in merges), (family, "a merge that appends drops a selection", merges)
        for sd in SEEDS:  # (in every sequence: the selection the chain makes is there at the move's and the ICP queries)
            held = [r[0]["state"]["selection"] for r in nm.replay(sd, family)
                    if r[0]["call"] == "query" and r[0]["edge"] in ("icp", "icp_again")]
            assert held == [True, True], (family, sd, held)
        # the ICP step: the same record behind a move of every point, on the given points of BEFORE the move
        for sd in SEEDS:
            rp = nm.replay(sd, family)
            again = [i for i, r in enumerate(rp) if r[0]["edge"] == "icp_again"]
            assert len(again) == 1, (family, sd)
            i = again[0]
            first, move = rp[i - 2], rp[i - 1]
            assert move[0]["call"] == "transform" and move[0]["sel"] is None and rp[i][0]["given"] == {"ref": i - 2}
            assert rp[i][1]["G"] is first[1]["G"] and first[0]["outputs"] == rp[i][0]["outputs"] == "both"
            assert rp[i][0]["radius"] == first[0]["radius"] and first[0]["given"]["m"] == len(first[1]["G"])
            # the reordered query: the answers of the query before the sort, array for array
            for j, r in enumerate(rp):
                if r[0]["edge"] == "reordered":
                    assert rp[j - 1][0]["call"] == "reorder" and rp[j - 3][0]["edge"] == "append_copies_sorted"
                    assert _states(family, sd)[j - 3].sorted, (family, sd, j, "appended onto a sorted cloud")
                    assert not nm.mismatches(nm.outputs(r[0], r[2]), nm.outputs(rp[j - 2][0], rp[j - 2][2])), (family, sd, j)
        # a copy and its original in different chunks of upload order
        apart = 0
        for fam, sd, i, rec, args, res, n0 in _steps(family, "append_copies"):
            apart += int((args["src"] // em.CHUNK != (n0 + np.arange(args["src"].size)) // em.CHUNK).sum())
            assert 64 <= rec["count"] <= 300 and args["src"].size == rec["count"] + rec["count"] // 3
            assert np.isfinite(args["xyz"]).all()
        assert apart >= 8, (family, apart)
    every = [s[3] for s in _steps()]
    assert {r["given"]["m"] for r in every if "m" in r["given"]} >= set(nm.GIVEN_COUNTS)
    assert any(r["kind"] == "nearest_k" and r["k"] > r["state"]["finite"] > 0 for r in every)
    assert any(r["state"]["chunks"] == 1 for r in every)


# ---- ties -----------------------------------------------------------------------------------------------------------------------
def _tied(xyz, G, radius):
    """bool (m,): the given points with two or more resident points at their bitwise-minimal d2, and the two first."""
    idx, d2, found, _ = nearest_k_ref.nearest_k_brute(xyz, G, radius, 2)
    b = d2.view(np.uint32)
    return (found >= 2) & (b[:, 0] == b[:, 1]), idx


def _renumber(bits):
    """old upload index -> new upload index behind a removal with keep bits `bits` (NONE: removed)."""
    new = (np.cumsum(bits) - 1).astype(np.uint32)
    new[~bits] = NONE
    return np.concatenate([new, np.full(1, NONE, np.uint32)])  # (NONE itself maps to NONE)


def _through(idx, table):
    return table[np.minimum(idx.astype(np.int64), len(table) - 1)]


def test_ties_under_renumbering():
    for family in sorted(FAMILIES):
        can_sort = em.allows_reorder(family) or FAMILIES[family].get("auto_reorder") == 1
        count = {k: 0 for k in QUERIES}
        apart = on_sorted = renumbered = 0
        for fam, sd, i, rec, args, res, n0 in _good(family):
            if rec["edge"] not in TIE_EDGES:
                continue
            states = _states(fam, sd)
            tied, idx = _tied(states[i].xyz, args["G"], rec["radius"])
            if tied.sum() >= 8:
                count[rec["kind"]] += 1
                apart += int((idx[tied, 0] // em.CHUNK != idx[tied, 1] // em.CHUNK).sum()) >= 8
                on_sorted += bool(rec["state"]["sorted"])
            if rec["edge"] == "survivors":  # (the winners on the cloud before the removal, through the survivors' indices)
                assert nm.sequence(sd, fam)[i - 1]["call"] == "remove_originals"
                bits = nm.replay(sd, fam)[i - 1][1]["bits"]
                was = nearest_ref.nearest_brute(states[i - 1].xyz, args["G"], rec["radius"])[0]
                now = res["all"][0] if rec["kind"] == "nearest" else res["index"][:, 0]
                differ = int((_through(was, _renumber(bits)) != now).sum())
                assert differ >= 8, (fam, sd, i, differ)
                renumbered += 1
        assert count["nearest"] >= 2 and count["nearest_k"] >= 2, (family, count)
        assert apart >= 1 and renumbered >= 1, (family, apart, renumbered)
        assert on_sorted >= 1 or not can_sort, family


# ---- shares ----------------------------------------------------------------------------------------------------------------------
def _differs(rec, args, res, prec, pargs, old, new):
    """Does the step's answer on the cloud as it was BEFORE the previous edit (stale coordinates where the point count
    is unchanged, a stale point set otherwise, laid beside the true one through the upload indices of the survivors)
    differ from `res`?"""
    was = nm.apply(old.copy(), rec, args)
    if was["error"] != res["error"]:
        return True
    if res["error"] is not None:
        return False
    a, b = nm.outputs(rec, was), nm.outputs(rec, res)
    a.pop("stats"), b.pop("stats")
    if old.n == new.n:
        pass  # (the same points, or an upload of as many: index by index)
    elif prec["call"] in REMOVALS:
        table = _renumber(pargs["bits"])
        for k in a:
            a[k] = _through(a[k], table) if k in ("given_index", "index") else a[k][pargs["bits"]] if k.startswith("resident") else a[k]
    else:
        assert prec["call"] in APPENDS, prec["call"]
        for k in b:
            b[k] = b[k][:old.n] if k.startswith("resident") else b[k]
    return bool(nm.mismatches(a, b))


def shares():
    """trivial steps / steps per kind (span steps excluded); k = 2 or 8 steps with a full and a partly filled row / such
    steps; stale-sensitive steps / query steps that follow an edit of coordinates or the point set; the same behind a
    reorder."""
    triv = {k: [0, 0] for k in nm.NEW}
    rows = [0, 0]
    for call in ("query", "merge"):
        for fam, sd, i, rec, args, res, n0 in _steps(call=call):
            if rec["edge"] in ("beyond_span", "at_span") or res["error"] is not None:
                continue
            kind = rec.get("kind", "merge")
            triv[kind][1] += 1
            triv[kind][0] += nm.trivial(rec, res)
            if kind == "nearest_k" and rec["k"] in (2, 8):
                f = res["found"]
                rows[1] += 1
                rows[0] += bool((f == rec["k"]).any() and ((f > 0) & (f < rec["k"])).any())
    stale, sort = [0, 0], [0, 0]
    for family, seed in CASES:
        states, rp = _states(family, seed), nm.replay(seed, family)
        for i in range(2, len(rp)):
            rec, args, res = rp[i][:3]
            prec, pargs = rp[i - 1][:2]
            if rec["call"] != "query" or prec["call"] in ("query", "set_keep", "clear_keep", "select"):
                continue
            old, new = states[i - 1], states[i]
            if prec["call"] == "reorder":
                sort[1] += 1
                sort[0] += _differs(rec, args, res, prec, pargs, old, new)
                continue
            if old.n == new.n and np.array_equal(old.xyz.view(np.uint32), new.xyz.view(np.uint32)):
                continue
            if old.n == 0 or (old.n != new.n and prec["call"] not in REMOVALS + APPENDS):
                continue  # (behind an empty cloud or an upload of another size nothing can be laid side by side: not counted)
            stale[1] += 1
            stale[0] += _differs(rec, args, res, prec, pargs, old, new)
    return triv, rows, stale, sort


def test_shares_stay_within_their_caps():
    triv, rows, stale, sort = shares()
    for kind in nm.NEW:
        t, n = triv[kind]
        print("trivial", kind, t, "of", n)
        assert n >= 18 and 4 * t <= n, (kind, t, n)
    print("full and partly filled rows", rows[0], "of", rows[1])
    assert rows[1] >= 18 and 3 * rows[0] >= rows[1], rows
    print("stale-sensitive", stale[0], "of", stale[1], "; behind a reorder", sort[0], "of", sort[1])
    assert stale[1] >= 100 and 2 * stale[0] >= stale[1], stale
    assert sort[0] == 0 and sort[1] >= 12, sort  # (the model has no resident order)
    ns = [s[6] for s in _steps()]
    print("points at the query steps", min(ns), "..", max(ns), "; query steps", len(ns), "; merges", triv["merge"][1])


# ---- the comparison can fail ----------------------------------------------------------------------------------------------------
def _largest_index_wins(rec, xyz, G):
    """The step's answer with every tie resolved to the LARGER index: the reference on the reversed cloud."""
    n, m = xyz.shape[0], nm.Model("pack0")
    m.xyz = np.ascontiguousarray(xyz[::-1])
    res = nm.apply(m, rec, {"G": G})
    flip = np.concatenate([np.arange(n - 1, -1, -1, dtype=np.uint32), np.full(1, NONE, np.uint32)])
    if rec["kind"] == "nearest":
        gi, gd, ri, rd = res["all"]
        res["given"] = (_through(gi, flip), gd) if res["given"] is not None else None
        res["resident"] = (ri[::-1], rd[::-1]) if res["resident"] is not None else None
    else:
        res["index"] = _through(res["index"], flip)
    return nm.outputs(rec, res)


def test_the_comparison_notices_each_kind_of_wrong_answer():
    for family in sorted(FAMILIES):
        seen = {"tie": 0, "renumber": 0, "row": 0, "quad": 0}
        for fam, sd, i, rec, args, res, n0 in _good(family):
            states, true = _states(fam, sd), nm.outputs(rec, res)
            assert nm.mismatches(true, nm.outputs(rec, res)) == []
            if rec["edge"] in TIE_EDGES:
                seen["tie"] += bool(nm.mismatches(_largest_index_wins(rec, states[i].xyz, args["G"]), true))
            if nm.sequence(sd, fam)[i - 1]["call"] in REMOVALS and states[i - 1].n != states[i].n:
                was = nm.outputs(rec, nm.apply(states[i - 1].copy(), rec, args))
                if rec["kind"] == "nearest" and "resident_index" in was:  # (as many entries as points are left)
                    bits = nm.replay(sd, fam)[i - 1][1]["bits"]
                    was["resident_index"], was["resident_dist2"] = was["resident_index"][bits], was["resident_dist2"][bits]
                seen["renumber"] += bool(set(nm.mismatches(was, true)) & {"given_index", "index"})
            if rec["kind"] == "nearest_k" and (res["found"] > 0).any():
                alt = {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in true.items()}
                j = int(np.flatnonzero(res["found"] > 0)[-1])
                alt["found"][j] -= 1
                alt["index"][j, alt["found"][j]], alt["dist2"][j, alt["found"][j]] = NONE, np.inf
                seen["row"] += set(nm.mismatches(alt, true)) == {"index", "dist2", "found"}
            if "resident_index" in true and n0 >= 4:
                alt = dict(true)
                alt["resident_index"] = np.concatenate([true["resident_index"][:-4], np.roll(true["resident_index"][-4:], 1)])
                alt["resident_dist2"] = np.concatenate([true["resident_dist2"][:-4], np.roll(true["resident_dist2"][-4:], 1)])
                seen["quad"] += bool(nm.mismatches(alt, true))
        assert all(v >= 1 for v in seen.values()), (family, seen)
