"""The checker and the inputs of test_gpu_rows_sequences.py, without a GPU, over exactly the seeds, families and step
count the GPU file runs: the four older generators' sequences are what they were (pinned digests); the model's
brute-force rows agree with the references' bucket forms, with nearest_k_ref's rows and with each other, and the
clean-up with the removal written out; the reference meets README_normals.md's two conditions on every normals step;
every call meets the states and the directed edits the device code branches on; ties at the rows' ends, trivial steps,
full and partly filled rows and the sensitivity to a stale cloud are measured against their caps
(tests/README_rows_sequences.md); and the GPU file's one comparison notices each way in which an answer could be subtly
wrong."""
import functools

import numpy as np

import analysis_model as am
import edit_model as em
import nearest_k_ref
import nearest_model as nm
import normals_ref as nf
import rows_model as rm
import select_ref
import statistical_ref as sf
import write_model as wm
from rows_model import CALLS, FAMILIES, KINDS, SEEDS, STEPS
from test_analysis_model_host import EDIT_DIGEST, WRITE_DIGEST, _digest
from test_nearest_model_host import ANALYSIS_DIGEST, NEAREST_DIGEST, _renumber, _through

CASES = [(family, seed) for family in sorted(FAMILIES) for seed in SEEDS]
f32 = np.float32
TIE_EDGES = ("copies", "survivors", "reordered")
SPAN = ("beyond_span", "at_span")
VALUES = {"statistical": ("mean", "found"), "normals": ("normals", "curvature", "found")}
# sha256 of repr() of every sequence of rows_model
ROWS_DIGEST = "4fdb3041e4a9ce8513d928a742b1a1a3e1a671756abe139a4387c93daa0ac72d"


def _steps(family=None):
    """(family, seed, step index, record, arguments, result, n before) of every rows step of the named sequences."""
    for fam, sd in CASES:
        if family is None or fam == family:
            for i, (rec, args, res, n0, s0, s1) in enumerate(rm.replay(sd, fam)):
                if rec["call"] == "rows":
                    yield fam, sd, i, rec, args, res, n0


def _good(family=None, kind=None):
    return [s for s in _steps(family) if s[5]["error"] is None and (kind is None or s[3]["kind"] == kind)]


@functools.lru_cache(maxsize=None)
def _states(family, seed):
    """The model before every step of a sequence, and after the last (a rows step through its cached result)."""
    model, out, past = rm.Model(family), [], []
    for rec, args, res, n0, s0, s1 in rm.replay(seed, family):
        out.append(model.copy())
        if rec["call"] == "rows":
            rm.advance(model, rec, res)
        else:
            rm.apply(model, rec, args)
    return out + [model.copy()]


def _full(rec):
    """The record with every output asked for: the comparisons below are about values, not about placement."""
    return dict(rec, place={name: "host" for name in rm.ARRAYS[rec["kind"]]}) if rec["kind"] in CALLS else rec


def _kept_bits(rec, args, res):
    """The keep bits of a step that removes points (None: it is none)."""
    if rec["call"] in ("remove", "remove_originals"):
        return args["bits"]
    if rec["call"] == "rows" and rec["kind"] == "cleanup" and res["error"] is None:
        return res["hit"]
    return None


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_the_older_sequences_are_unchanged():
    assert _digest(em, em.FAMILIES) == EDIT_DIGEST
    assert _digest(wm, wm.WRITE_FAMILIES) == WRITE_DIGEST
    assert _digest(am, am.FAMILIES) == ANALYSIS_DIGEST
    assert _digest(nm, nm.FAMILIES) == NEAREST_DIGEST
    assert _digest(rm, rm.FAMILIES) == ROWS_DIGEST


def test_sequences_are_a_pure_function_of_their_arguments():
    for family, seed in CASES:
        a = rm.sequence(seed, family, STEPS)
        assert len(a) == STEPS and a[0]["call"] == "upload", (family, seed)
        if (seed, family) == (SEEDS[0], "specials"):  # (drawn again, past the cache)
            assert a == tuple(r[0] for r in rm._replay.__wrapped__(seed, family, STEPS)), (family, seed)
        assert rm.sequence(seed, family, 10) == a[:10], (family, seed)  # (a prefix reproduces a failure)
    assert (SEEDS, STEPS) == ((1, 2, 3), 30) and set(FAMILIES) == set(em.FAMILIES) and len(CASES) == 18 and rm.REGRESSIONS == {}


def test_records_say_where_they_stand():
    for family, seed in CASES:
        recs, states = rm.sequence(seed, family), _states(family, seed)
        for i, rec in enumerate(recs):
            assert states[i].n <= em.N_MAX
            if rec["call"] == "rows":
                prev = recs[i - 1]
                assert rec["state"]["after"] == (prev["kind"] if prev["call"] == "rows" else prev["call"]), (family, seed, i)
                assert rec["state"]["after_edge"] == prev["edge"], (family, seed, i)
                assert rec["state"]["n"] == states[i].n and rec["state"]["sorted"] == states[i].sorted, (family, seed, i)
                assert 1 <= rec["k"] <= 64 and (rec["kind"] == "cleanup" or set(rec["place"]) == set(rm.ARRAYS[rec["kind"]]))
            if rec["edge"] in rm.SHARED + ("append_empty", "append_mirrors", "remove_originals", "append_copies_sorted", "reorder",
                                           "append_one", "remove_last_point", "cleanup", "cleanup_again"):
                if rec["edge"] != "remove_all_then_append":  # (its append comes first)
                    assert i + 1 < len(recs) and recs[i + 1]["call"] == "rows" and recs[i + 1]["kind"] in CALLS, (family, seed, i)
        assert not (recs[-1]["call"] == "rows" and recs[-1]["kind"] == "cleanup" and recs[-1]["edge"] not in SPAN), (family, seed)


# ---- the model against the definitions -------------------------------------------------------------------------------------
def test_brute_rows_agree_with_the_bucket_forms():
    done = refused = 0
    for fam, sd, i, rec, args, res, n0 in _good():
        if rec["kind"] == "cleanup":
            continue
        xyz, r, k = _states(fam, sd)[i].xyz, rec["radius"], rec["k"]
        try:
            if rec["kind"] == "normals":
                idx, d2, found = nf.rows_bucket(xyz, r, k)
                assert np.array_equal(idx, res["index"]) and nf.same_bits(d2, res["d2"]) and np.array_equal(found, res["found"]), (fam, sd, i)
            else:
                rows, found = sf.rows_bucket(xyz, r, k)
                assert np.array_equal(found, res["found"]) and nf.same_bits(sf.means(rows, found), res["mean"]), (fam, sd, i)
        except ValueError:  # (the bucket forms' own grid, anchored elsewhere, ends a little before the library's span does)
            assert rec["edge"] == "at_span", (fam, sd, i)
            refused += 1
            continue
        done += 1
    assert done >= 200 and refused <= 36, (done, refused)


def test_normals_rows_are_the_nearest_k_rows_without_the_own_index():
    for family in sorted(FAMILIES):
        fam, sd, i, rec, args, res, n0 = min((s for s in _good(family, "normals") if s[3]["edge"] in TIE_EDGES), key=lambda s: s[6])
        xyz = _states(fam, sd)[i].xyz
        index, d2, found, _ = nearest_k_ref.nearest_k_brute(xyz, xyz, rec["radius"], rec["k"] + 1)
        idx, rows, fd = nf.rows_from_nearest_k(index, d2, found, rec["k"])
        assert np.array_equal(idx, res["index"]) and nf.same_bits(rows, res["d2"]) and np.array_equal(fd, res["found"]), (fam, sd, i)


def test_both_calls_find_the_same_rows_and_the_cleanup_is_the_removal_written_out():
    pairs = cleanups = 0
    for family, seed in CASES:
        rp, states = rm.replay(seed, family), _states(family, seed)
        for i, (rec, args, res, n0, s0, s1) in enumerate(rp):
            if rec["call"] != "rows" or res["error"] is not None:
                continue
            if rec["kind"] == "statistical" and i and rp[i - 1][0]["call"] == "rows" and rp[i - 1][0]["kind"] == "normals" and \
                    (rp[i - 1][0]["k"], rp[i - 1][0]["radius"]) == (rec["k"], rec["radius"]) and rp[i - 1][2]["error"] is None:
                assert np.array_equal(res["found"], rp[i - 1][2]["found"]), (family, seed, i)
                pairs += 1
            if rec["kind"] == "cleanup":
                before, after = states[i], states[i + 1]
                s = sf.select(before.xyz, rec["radius"], rec["k"], rec["std_mul"])  # (statistical_ref's own rows)
                assert np.array_equal(s["hit"], res["hit"]) and res["removed"] == int((~s["hit"]).sum()), (family, seed, i)
                fin = np.isfinite(before.xyz).all(axis=1)
                assert not s["hit"][~fin].any() and not s["hit"][s["found"] == 0].any()  # (non-finite and isolated points go)
                want = em.Model(family)
                want.__dict__.update(em.Model.copy(before).__dict__)
                want.remove(s["hit"])
                assert np.array_equal(after.xyz.view(np.uint32), want.xyz.view(np.uint32)) and np.array_equal(after.rgb, want.rgb)
                assert after.selection is None and (after.keep is None) == (want.keep is None), (family, seed, i)
                assert want.keep is None or np.array_equal(after.keep, want.keep)
                cleanups += 1
    assert pairs >= 18 and cleanups >= 18, (pairs, cleanups)


def test_span_steps_sit_where_they_say():
    for fam, sd, i, rec, args, res, n0 in _steps():
        if rec["edge"] not in SPAN:
            continue
        before, after = _states(fam, sd)[i], _states(fam, sd)[i + 1]
        xyz = before.xyz
        fin = xyz[np.isfinite(xyz).all(axis=1)]
        far = rm.beyond_span(xyz, rec["radius"])
        if rec["edge"] == "beyond_span":
            assert far.any() and res["error"] == "unsupported", (fam, sd, i)
            assert after.n == before.n and np.array_equal(after.xyz.view(np.uint32), xyz.view(np.uint32))  # (nothing removed)
            assert (after.selection is None) == (before.selection is None)
        else:
            assert not far.any() and res["error"] is None and rm.axis_in_span(fin, rec["radius"]).all(), (fam, sd, i)
            q = np.abs(np.floor(fin.astype(np.float64) / am.cell_edge(rec["radius"])))
            assert q.max() >= 0.98 * 2 ** 20, (fam, sd, i)  # (the outermost points lie in the last cells)


def test_the_reference_meets_its_two_conditions_on_every_normals_step():
    """README_normals.md's conditions, with test_normals_host.py's bounds (they are literals there): after the 8th
    sweep every off-diagonal entry is 0, and the Rayleigh quotient of the fp32 normal exceeds eigh's smallest
    eigenvalue by at most 2^-40 of the trace."""
    worst, seen = 0.0, 0
    for fam, sd, i, rec, args, res, n0 in _good(kind="normals"):
        have = res["found"] >= nf.MIN_FOUND
        if not have.any():
            continue
        Cm = res["C"][have]
        tr = Cm[:, 0, 0] + Cm[:, 1, 1] + Cm[:, 2, 2]
        A, _ = nf.jacobi(Cm)
        off = np.max(np.abs(np.stack([A[:, 0, 1], A[:, 0, 2], A[:, 1, 2]], 1)), axis=1)
        assert (off == 0.0).all(), (fam, sd, i, float(off.max()))
        lam, _ = nf.eigh_of(Cm)
        n64 = res["normals"][have].astype(np.float64)
        ray = np.einsum("ni,nij,nj->n", n64, Cm, n64) / np.einsum("ni,ni->n", n64, n64)
        assert (ray - lam[:, 0] <= 2.0 ** -40 * tr).all(), (fam, sd, i, float(((ray - lam[:, 0]) / np.where(tr > 0, tr, 1)).max()))
        worst = max(worst, float(((ray - lam[:, 0]) / np.where(tr > 0, tr, 1)).max()))
        seen += int(have.sum())
    print("neighbourhoods", seen, "; worst Rayleigh excess / trace", worst)
    assert seen >= 100_000


# ---- the chains ---------------------------------------------------------------------------------------------------------------
def _values(rec, res, keep=None, head=None):
    """The per-point outputs of a step, on the points `keep` names or on the first `head`."""
    out = {}
    for name in VALUES[rec["kind"]]:
        a = res[name]
        out[name] = a[keep] if keep is not None else a[:head] if head is not None else a
    return out


def test_the_chains_do_what_they_are_for():
    for family in sorted(FAMILIES):
        sorted_twice = same_n = given = selected = 0
        for sd in SEEDS:
            rp, states = rm.replay(sd, family), _states(family, sd)
            for i, (rec, args, res, n0, s0, s1) in enumerate(rp):
                edge = rec["edge"]
                if rec["call"] != "rows":
                    continue
                if edge == "reordered":  # (the same record on both sides of a sort of a cloud copies were appended to sorted)
                    assert rp[i - 1][0]["call"] == "reorder" and rp[i - 3][0]["edge"] == "append_copies_sorted" and states[i - 3].sorted
                    assert {k: v for k, v in rp[i - 2][0].items() if k not in ("edge", "state")} == \
                           {k: v for k, v in rec.items() if k not in ("edge", "state")}
                    assert rm.mismatches(rm.outputs(rec, res), rm.outputs(rec, rp[i - 2][2])) == [], (family, sd, i)
                    sorted_twice += 1
                if edge == "survivors":
                    assert rp[i - 1][0]["call"] == "remove_originals" and rp[i - 2][0]["edge"] == "copies" and \
                        [r[0]["call"] for r in rp[i - 4:i - 2]] == ["append_copies", "append_mirrors"]
                    assert rec["k"] in rm.COPY_KS and rec["radius"] == rp[i - 2][0]["radius"], (family, sd, i)
                if edge == "copies":  # (a point copied twice has a row that starts with its two copies at d2 = +0)
                    j = i - 1 if rp[i - 1][0]["call"] != "append_mirrors" else i - 2
                    src, count = rp[j][1]["src"], rp[j][0]["count"]
                    twice = rp[j][3] + count + np.arange(count // 3)
                    assert rp[j][0]["call"] == "append_copies" and src.size == count + count // 3
                    assert not res["d2"][twice, :2].view(np.uint32).any() and (res["found"][twice] >= 2).all(), (family, sd, i)
                if edge == "same_n_again":
                    a, b, c = rp[i - 4], rp[i - 2], rp[i]
                    assert [r[0]["edge"] for r in rp[i - 4:i + 1]] == ["same_n", "append_one", "same_n_plus_1", "remove_last_point", "same_n_again"]
                    assert a[3] == c[3] == b[3] - 1 and all(r[0]["place"]["mean"] and r[0]["place"]["found"] for r in (a, b, c))
                    assert np.array_equal(states[i - 4].xyz.view(np.uint32), states[i].xyz.view(np.uint32))
                    assert rm.mismatches(rm.outputs(a[0], a[2]), rm.outputs(c[0], c[2])) == [], (family, sd, i)
                    changed = (a[2]["mean"].view(np.uint32) != b[2]["mean"][:a[3]].view(np.uint32)) | (a[2]["found"] != b[2]["found"][:a[3]])
                    assert changed.any(), (family, sd, i, "the appended point entered a row")
                    same_n += 1
                if edge == "selected" and rec["kind"] == "statistical":
                    assert s0 is not None and rec["op"] in rm.COMBINING and rp[i + 1][0]["kind"] == "normals", (family, sd, i)
                    nrm = rp[i + 1]
                    assert nrm[4] is not None and np.array_equal(nrm[4], nrm[5])  # (normals: the selection's bits stay)
                    selected += 1
                if edge == "given":
                    assert rec["threshold"] is not None and s0 is not None, (family, sd, i)
                    first = [r for r in rp[:i] if r[0]["edge"] == "selected" and r[0].get("kind") == "statistical"][-1]
                    assert rec["threshold"] == first[2]["moments"][2] == res["moments"][2], (family, sd, i)
                    assert res["moments"][:2] == sf.moments(res["mean"], res["found"], 1.0)[:2]
                    given += 1
        assert same_n >= 1 and selected >= 1 and given >= 1, (family, same_n, selected, given)
        assert sorted_twice >= 1 or not em.allows_reorder(family), family
    for rec, args, res, n0, s0, s1 in (r for c in CASES for r in rm.replay(c[1], c[0])):  # (normals never makes a selection)
        if rec["call"] == "rows" and rec["kind"] == "normals":
            assert (s0 is None) == (s1 is None) and (s0 is None or np.array_equal(s0, s1))


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
        for kind in CALLS:
            for edge in SPAN:  # (once in every sequence)
                need(sorted(s[1] for s in steps if s[3]["kind"] == kind and s[3]["edge"] == edge) == list(SEEDS), (family, kind, edge))
            got = {s[3]["k"] for s in _good(family, kind)}
            need(got >= set(rm.KS), (family, kind, "every k", sorted(set(rm.KS) - got)))
        need(sum(s[3]["kind"] == "cleanup" and s[3]["edge"] == "beyond_span" for s in steps) == 1, (family, "cleanup beyond_span"))
        # every followed edit has a step of one of the two calls directly behind it (test_records_say_where_they_stand)
        after = {s[3]["state"]["after_edge"] for s in steps if s[3]["kind"] in CALLS}
        want = set(rm.SHARED) - {"remove_all_then_append"} | {"append_empty", "append_mirrors", "remove_originals", "append_one",
                                                             "remove_last_point", "cleanup"}
        if em.allows_reorder(family):
            want |= {"reorder", "append_copies_sorted"}
        need(want <= after, (family, "edits a call follows directly", sorted(want - after)))
        # each call behind every followed edit: in the run of steps of the two calls that stands directly behind it
        behind = {k: set() for k in CALLS}
        for sd in SEEDS:
            rp = rm.replay(sd, family)
            for i, r in enumerate(rp):
                if r[0]["call"] != "rows" and r[0]["edge"] in rm.SHARED + ("append_empty",):
                    j = i + 1
                    while j < len(rp) and rp[j][0]["call"] == "rows" and rp[j][0]["kind"] in CALLS and rp[j][2]["error"] is None:
                        behind[rp[j][0]["kind"]].add(r[0]["edge"])
                        j += 1
                if r[0]["edge"] == "append_empty":
                    emptied.add(r[0]["m"])
        for kind in CALLS:
            lack = set(rm.SHARED) - {"remove_all_then_append"} | {"append_empty"}
            need(behind[kind] >= lack, (family, kind, "behind every followed edit", sorted(lack - behind[kind])))
        good = _good(family)
        stat = [s[3] for s in good if s[3]["kind"] == "statistical"]
        need({r["op"] for r in stat} == set(em.OPS) and any(r["outside"] for r in stat), (family, "ops", sorted({r["op"] for r in stat})))
        need(any(r["threshold"] is not None for r in stat), (family, "a given threshold"))
        need({r["std_mul"] for r in stat} == set(rm.STD_MULS), (family, "std_mul"))
        nrm = [s for s in good if s[3]["kind"] == "normals"]
        need(any(s[3]["state"]["selection"] for s in nrm), (family, "a selection in force at a normals step"))
        need(any(s[3]["viewpoint"] is not None for s in nrm) and any(s[3]["viewpoint"] is None for s in nrm), (family, "viewpoint"))
        need(any((s[5]["found"] < 2).any() for s in nrm), (family, "a point with found < 2"))
        need(any((s[5]["found"] >= 2).all() for s in nrm), (family, "every point with found >= 2"))
    need(emptied == set(rm.EMPTY_APPEND), ("the appends behind a removal of every point", sorted(emptied)))
    again = sum(s[3]["edge"] == "cleanup_again" and s[5]["error"] is None for s in _steps())
    need(again >= 1, ("a second clean-up among the random steps", again))
    every = [s for s in _steps()]
    for kind in CALLS:  # (output placement is independent for each array: every combination occurs)
        got = {tuple(s[3]["place"][a] for a in rm.ARRAYS[kind]) for s in every if s[3]["kind"] == kind}
        want = {()}
        for _ in rm.ARRAYS[kind]:
            want = {w + (p,) for w in want for p in rm.PLACES}
        need(got == want, (kind, "placements that never occur", sorted(want - got, key=str)))
    stat_n = {s[6] % 256 for s in every if s[3]["kind"] == "statistical" and s[5]["error"] is None}
    need({0, 1, 255} <= stat_n, sorted(stat_n))
    need(any(s[3]["k"] > s[3]["state"]["finite"] > 0 for s in every), "n < k")
    need(any(s[3]["state"]["chunks"] == 1 for s in every), "a one-chunk cloud")
    crossed = 0
    for family, seed in CASES:
        ns = [s[6] for s in _steps(family) if s[1] == seed and s[3]["kind"] == "statistical" and s[5]["error"] is None]
        crossed += sum(a // 1024 != b // 1024 for a, b in zip(ns, ns[1:]))
    need(crossed >= 1, "a cloud crosses a multiple of 1024 between two statistical steps")
    eyes = 0
    for family, seed in CASES:  # (pose_for's eye position, once per sequence)
        states = _states(family, seed)
        eyes += any(s[3]["kind"] == "normals" and s[3]["viewpoint"] is not None and
                    np.array_equal(f32(s[3]["viewpoint"]), rm.eye_of(rm.pose_for(states[s[2]], s[2])).astype(f32))
                    for s in _steps(family) if s[1] == seed)
    need(eyes == len(CASES), eyes)
    assert missing == [], "\n".join(repr(m) for m in missing)


# ---- ties at the rows' ends ---------------------------------------------------------------------------------------------------
def _end_ties(xyz, rec):
    """bool (n,): the points whose last kept entry ties in d2 bits with the first one that was dropped."""
    _, d2, found = rm.rows_of(xyz, rec["radius"], rec["k"] + 1)
    b = d2.view(np.uint32)
    return (found >= rec["k"] + 1) & (b[:, rec["k"] - 1] == b[:, rec["k"]])


def test_ties_at_the_rows_ends_under_renumbering():
    for family in sorted(FAMILIES):
        tied = renumbered = 0
        for fam, sd, i, rec, args, res, n0 in _good(family, "normals"):
            if rec["edge"] not in TIE_EDGES:
                continue
            states = _states(fam, sd)
            many = int(_end_ties(states[i].xyz, rec).sum()) >= 8
            tied += many
            if rec["edge"] == "survivors":  # (the rows on the cloud before the removal, through the survivors' indices)
                bits = rm.replay(sd, fam)[i - 1][1]["bits"]
                was = nf.cut(rm.rows_of(states[i - 1].xyz, rec["radius"], rec["k"]), rec["k"])[0][bits]
                differ = int((_through(was, _renumber(bits)) != res["index"]).any(axis=1).sum())
                assert differ >= 8, (fam, sd, i, differ)
                renumbered += many
        assert tied >= 2 and renumbered >= 1, (family, tied, renumbered)


# ---- shares ----------------------------------------------------------------------------------------------------------------------
def _differs(rec, args, res, old, bits, n_new):
    """Does the step's answer on the cloud as it was BEFORE the previous edit (stale coordinates where the point count
    is unchanged, a stale point set otherwise) differ from `res` on the points both clouds hold?"""
    was = rm.apply(old.copy(), _full(rec), args)
    if was["error"] != res["error"]:
        return True
    if res["error"] is not None:
        return False
    if old.n == n_new:
        a, b = _values(rec, was), _values(rec, res)
    elif bits is not None:
        a, b = _values(rec, was, keep=bits), _values(rec, res)
    else:
        a, b = _values(rec, was), _values(rec, res, head=old.n)
    return any(not rm._same_array(a[k], b[k]) for k in a)


def shares():
    """trivial steps / steps per kind (span steps excluded); normals steps of the copies' k with a full and a partly
    filled row / such steps; stale-sensitive steps / steps of the two calls that follow an edit of coordinates or the
    point set; the same behind a reorder."""
    triv = {k: [0, 0] for k in KINDS}
    rows = [0, 0]
    for fam, sd, i, rec, args, res, n0 in _good():
        if rec["edge"] in SPAN:
            continue
        triv[rec["kind"]][1] += 1
        triv[rec["kind"]][0] += rm.trivial(rec, res)
        if rec["kind"] == "normals" and rec["k"] in rm.COPY_KS:
            f = res["found"]
            rows[1] += 1
            rows[0] += bool((f == rec["k"]).any() and ((f > 0) & (f < rec["k"])).any())
    stale, sort = [0, 0], [0, 0]
    for family, seed in CASES:
        states, rp = _states(family, seed), rm.replay(seed, family)
        for i in range(2, len(rp)):
            rec, args, res = rp[i][:3]
            prec, pargs, pres = rp[i - 1][:3]
            if rec["call"] != "rows" or rec["kind"] not in CALLS or rec["edge"] in SPAN:
                continue
            if prec["call"] in ("set_keep", "clear_keep", "select") or (prec["call"] == "rows" and prec["kind"] != "cleanup"):
                continue
            old, new = states[i - 1], states[i]
            bits = _kept_bits(prec, pargs, pres)
            if prec["call"] == "reorder":
                sort[1] += 1
                sort[0] += _differs(rec, args, res, old, None, new.n)
                continue
            if old.n == new.n and np.array_equal(old.xyz.view(np.uint32), new.xyz.view(np.uint32)):
                continue
            if old.n == 0 or (old.n != new.n and bits is None and prec["call"] not in ("append", "append_copies", "append_near", "append_mirrors")):
                continue  # (behind an empty cloud or an upload of another size nothing can be laid side by side: not counted)
            stale[1] += 1
            stale[0] += _differs(rec, args, res, old, bits, new.n)
    return triv, rows, stale, sort


def test_shares_stay_within_their_caps():
    triv, rows, stale, sort = shares()
    for kind in KINDS:
        t, n = triv[kind]
        print("trivial", kind, t, "of", n)
        assert n >= 18 and 4 * t <= n, (kind, t, n)
    print("full and partly filled rows", rows[0], "of", rows[1])
    assert rows[1] >= 18 and 3 * rows[0] >= rows[1], rows
    print("stale-sensitive", stale[0], "of", stale[1], "; behind a reorder", sort[0], "of", sort[1])
    assert stale[1] >= 100 and 2 * stale[0] >= stale[1], stale
    assert sort[0] == 0 and sort[1] >= 4, sort  # (the model has no resident order; once in every family that sorts)
    ns = [s[6] for s in _steps()]
    print("points at the rows steps", min(ns), "..", int(np.median(ns)), "..", max(ns), "; rows steps", len(ns))


# ---- the comparison can fail ----------------------------------------------------------------------------------------------------
def _larger_index_ends_the_row(rec, args, res, xyz):
    """(the step's answer, the rows changed) with the first DROPPED entry in the place of the last kept one in every row
    where the two have the same d2 bits -- the tie resolved to the larger index, nothing else in the row touched."""
    k = rec["k"]
    more, d2, found = nf.cut(rm.rows_of(xyz, rec["radius"], k + 1), k + 1)
    b = d2.view(np.uint32)
    tied = (found >= k + 1) & (b[:, k - 1] == b[:, k])
    idx = res["index"].copy()
    idx[tied, k - 1] = more[tied, k]
    e = nf.estimate(xyz, rec["radius"], k, args["viewpoint"], rows_k=(idx, res["d2"], res["found"]))
    return rm.outputs(rec, dict(res, normals=e["normals"], curvature=e["curvature"], stats=e["stats"])), tied


def _left_behind(true, bits):
    """Per-point outputs written at the indices the survivors had BEFORE the removal `bits`."""
    alt, old = dict(true), np.flatnonzero(bits)
    for k, v in true.items():
        if isinstance(v, np.ndarray) and k != "selection" and not k.startswith("_"):
            a = np.full_like(v, 7)
            ok = old < len(v)
            a[old[ok]] = v[ok]
            alt[k] = a
    return alt


def test_the_comparison_notices_each_kind_of_wrong_answer():
    for family in sorted(FAMILIES):
        seen = {"tie": 0, "renumber": 0, "row": 0, "chunk": 0, "slot": 0, "tail": 0}
        for fam, sd, i, rec, args, res, n0 in _good(family):
            if rec["kind"] == "cleanup":
                continue
            rec = _full(rec)
            rp, states, true = rm.replay(sd, fam), _states(fam, sd), rm.outputs(rec, res)
            xyz = states[i].xyz
            assert rm.mismatches(true, rm.outputs(rec, res)) == []
            prec, pargs, pres = rp[i - 1][:3]
            if rec["edge"] in TIE_EDGES and rec["kind"] == "normals" and not seen["tie"]:
                alt, tied = _larger_index_ends_the_row(rec, args, res, xyz)
                moved = (alt["normals"].view(np.uint32) != true["normals"].view(np.uint32)).any(axis=1)
                assert not moved[~tied].any()  # (only the rows whose end was swapped answer differently)
                seen["tie"] += moved.any() and "normals" in rm.mismatches(alt, true)
            bits = _kept_bits(prec, pargs, pres)
            if bits is not None and not bits.all() and bits.any() and not seen["renumber"]:
                seen["renumber"] += bool(rm.mismatches(_left_behind(true, bits), true))
            if rec["kind"] == "normals" and (res["found"] >= 3).any() and not seen["row"]:
                j = int(np.flatnonzero(res["found"] >= 3)[-1])
                idx, d2, found = res["index"].copy(), res["d2"].copy(), res["found"].copy()
                found[j] -= 1
                idx[j, found[j]], d2[j, found[j]] = nf.NONE, np.inf
                e = nf.estimate(xyz, rec["radius"], rec["k"], args["viewpoint"], rows_k=(idx, d2, found))
                alt = rm.outputs(rec, dict(res, normals=e["normals"], curvature=e["curvature"], found=e["found"], stats=e["stats"]))
                seen["row"] += {"found", "normals"} <= set(rm.mismatches(alt, true))
            if prec["call"] == "transform" and seen["chunk"] < 1:
                moved = np.flatnonzero(np.ones(n0, bool) if pargs["bits"] is None else pargs["bits"])
                for c in np.unique(moved // em.CHUNK)[:3]:
                    m = states[i].copy()
                    m.xyz[c * em.CHUNK:(c + 1) * em.CHUNK] = states[i - 1].xyz[c * em.CHUNK:(c + 1) * em.CHUNK]
                    if rm.mismatches(rm.outputs(rec, rm.apply(m, rec, args)), true):
                        seen["chunk"] += 1
                        break
            if not seen["slot"] and n0 >= 3:
                hit = 0
                for name in VALUES[rec["kind"]]:
                    for shift in (1, -1):
                        alt = dict(true)
                        alt[name] = np.roll(true[name], shift, axis=0)
                        hit += rm.mismatches(alt, true) == [name]
                seen["slot"] += hit == 2 * len(VALUES[rec["kind"]])
            if rec["kind"] == "statistical" and n0 % 64 and res["selection"][64 * (n0 // 64):].any() and not seen["tail"]:
                sel = res["selection"].copy()
                sel[64 * (n0 // 64):] = False
                seen["tail"] += rm.mismatches(dict(true, selection=select_ref.words(sel)), true) == ["selection"]
        assert all(v >= 1 for v in seen.values()), (family, sorted(seen.items()))
    # the moments: within the tolerance they pass, beyond it they fail, and a t that moves a hit is a wrong hit
    fam, sd, i, rec, args, res, n0 = next(s for s in _good(kind="statistical") if 0 < s[5]["hit"].sum() < s[6] and not s[5]["given"])
    true = rm.outputs(_full(rec), res)
    mu, sigma, t = true["moments"]
    assert rm.mismatches(dict(true, moments=(mu * (1 + 2.0 ** -50), sigma, t)), true) == []
    assert rm.mismatches(dict(true, moments=(mu * (1 + 2.0 ** -30), sigma, t)), true) == ["moments"]
    edge = float(np.sort(res["mean"][res["hit"]].astype(np.float64))[-1])
    assert rm.mismatches(dict(true, moments=(mu, sigma, np.nextafter(edge, -np.inf))), true) in (["hit"], ["moments"])
