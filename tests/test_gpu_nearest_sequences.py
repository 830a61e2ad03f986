"""The nearest-point queries inside long chains of edits (include/rtr.h sections 6l and 6m): the seeded sequences of
nearest_model.py -- write_model's appends, removals, moves, masks, selections, sorts and writes with rtr_nearest_points,
rtr_nearest_k_points, ProjectCloud.matchPoints and ProjectCloud.appendNewPoints among them, a query directly behind every
edit that rewrites chunk boxes, populations, the permutation or the upload indices: copies appended beside their
originals, the originals removed, copies appended onto a sorted cloud, an ICP step -- on clouds of at most 8192 points,
driven on the library and on the host model.  After EVERY query every returned array (indices and found by value,
distances by their bits) and all four stats (matchPoints returns none) equal the model's, skipped + decoded chunks are the chunk count, and
test_gpu_edit_sequences.py's own checks follow (point count, option read-backs, keep and selection words, the extraction
of every point): the two calls leave the selection and the keep mask alone and create no selection.  A step the model
expects to fail raises RTR_ERR_UNSUPPORTED and changes nothing.  Frames and the point pass are checked after every fourth
step and at the end; at the end a second context with one upload of the model's cloud answers the last successful step
of every kind as the edited context does, and a last merge leaves both with the same cloud.
test_nearest_model_host.py checks the model, the coverage and the sensitivity of exactly these sequences without a GPU."""
import numpy as np
import pytest

import nearest_model as nm
import test_gpu_edit_sequences as es
import test_gpu_write_sequences as ws

pytestmark = pytest.mark.gpu


def _facade(pkg, p):
    """ProjectCloud's two calls on the context p (its constructor would make a context of its own and upload): the
    methods themselves on a stub that holds what they use, as test_near_host.py and test_nearest_host.py run them."""
    class Stub:
        _p = p
        appendPoints = pkg.ProjectCloud.appendPoints
        appendNewPoints = pkg.ProjectCloud.appendNewPoints
        nearestPoints = pkg.ProjectCloud.nearestPoints
        matchPoints = pkg.ProjectCloud.matchPoints
        _gather_matched = pkg.ProjectCloud._gather_matched
    return Stub()


def _rows(rec, G):
    """The given points as the record passes them: rows of 3 or 4 floats, host numpy or a device tensor."""
    rows = np.full((G.shape[0], rec["width"]), 7.5, np.float32)
    rows[:, :3] = G
    if rec["source"] == "host":
        return rows
    import torch
    return torch.from_numpy(rows).to(torch.device("cuda", 0))


def _host(rec, a):
    """A returned array on the host; device rows give tensors on the device, host rows numpy arrays."""
    if rec["source"] == "device":
        assert hasattr(a, "is_cuda") and a.is_cuda, "device input gives device output"
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray)
    return a


def _call(pkg, p, rec, args):
    """The record's query on the facade -> (nearest_model.outputs' dict of what it returned, (skipped, decoded))."""
    G = _rows(rec, args["G"])
    if rec["kind"] == "nearest_k":
        idx, d2, found, st = p.nearest_k_points(G, rec["k"], rec["radius"])
        got = {"index": _host(rec, idx), "dist2": _host(rec, d2), "found": _host(rec, found), "stats": st}
        return got, (p.get_option("nearest_k_chunks_skipped"), p.get_option("nearest_k_chunks_decoded"))
    if rec["match"]:
        idx, d2, xyz, rgb = _facade(pkg, p).matchPoints(G, rec["radius"])
        got = {"given_index": idx, "given_dist2": d2, "matched": (xyz, rgb)}
    else:
        out = p.nearest_points(G, rec["radius"], given=rec["outputs"] != "resident", resident=rec["outputs"] != "given")
        names = [s + e for s in ("given", "resident") if rec["outputs"] in (s, "both") for e in ("_index", "_dist2")]
        got = dict(zip(names, (_host(rec, a) for a in out[:-1])), stats=out[-1])
    return got, (p.get_option("nearest_chunks_skipped"), p.get_option("nearest_chunks_decoded"))


def _check_query(pkg, p, rec, args, res, model, what):
    """The record's query on the library against the model's result `res` (model: the state BEFORE the step)."""
    L = pkg._lib
    if res["error"] is not None:
        with pytest.raises(RuntimeError) as e:
            _call(pkg, p, rec, args)
        assert type(e.value) is pkg.RtrError and e.value.code == L.RTR_ERR_UNSUPPORTED, (str(e.value), what)
        return None
    got, chunks = _call(pkg, p, rec, args)
    want = nm.outputs(rec, res)
    matched = got.pop("matched", None)
    if matched is not None:  # (matchPoints: the winners' own coordinates and colours, zero where there is no match)
        want.pop("stats")
        idx, (xyz, rgb) = want["given_index"], matched
        hit = idx != nm.NONE
        assert xyz.shape == (len(idx), 3) and rgb.shape == (len(idx), 3) and rgb.dtype == np.uint8, what
        assert not xyz[~hit].view(np.uint32).any() and not rgb[~hit].any(), ("unmatched rows are zero", what)
        es._same_xyz(xyz[hit], model, idx[hit], ("matched coordinates", what))
        assert np.array_equal(rgb[hit], model.rgb[idx[hit]]), ("matched colours", what)
    assert nm.mismatches(got, want) == [], (nm.mismatches(got, want), got.get("stats"), want.get("stats"), what)
    assert chunks[0] + chunks[1] == (model.n + 255) // 256, ("chunks skipped + decoded", chunks, what)
    if rec["kind"] == "nearest_k" and rec["k"] == 1:  # (the ONE kernel against section 6l on the same inputs)
        gi, gd, st = p.nearest_points(_rows(rec, args["G"]), rec["radius"])
        assert np.array_equal(_host(rec, gi), got["index"][:, 0]), ("k = 1 against nearest_points: index", what)
        assert np.array_equal(_host(rec, gd).view(np.uint32), got["dist2"][:, 0].view(np.uint32)), ("k = 1: dist2", what)
        assert (st[0], st[2]) == (got["stats"][0], got["stats"][2]), ("k = 1: counts", st, got["stats"], what)
    return got, chunks


def _merge(pkg, p, rec, args):
    return _facade(pkg, p).appendNewPoints(args["G"], args["C"], rec["radius"])


def _drive(pkg, p, rec, args, model, what):
    call = rec["call"]
    if call == "append_copies":
        p.append_points(args["xyz"], args["rgb"])
    elif call == "remove_originals":
        p.remove_points(es._arg(pkg, p, rec["form"], ("originals",), args["bits"]))
    elif call == "write":
        ws._drive_write(pkg, p, rec, args, model, what)
    else:
        es._drive(pkg, p, rec, args, model, what)


def _check_repeats(pkg, p, model, family, last, what):
    """The last successful step of every kind again, on the edited context and on a context that uploads the model's
    cloud once: the same answers, array for array (the split between skipped and decoded chunks depends on the resident
    order: its sum).  The merge comes last, and both clouds are extracted afterwards: they are one cloud."""
    if model.n == 0:
        return
    b = es._new(pkg, family)
    try:
        b.upload_points(model.xyz, model.rgb)
        if model.keep is not None:
            b.set_point_keep(model.keep)
        for kind in nm.QUERIES:
            if kind in last:
                rec, args = last[kind]
                (ga, ca), (gb, cb) = _call(pkg, p, rec, args), _call(pkg, b, rec, args)
                ma, mb = ga.pop("matched", None), gb.pop("matched", None)
                assert nm.mismatches(ga, gb) == [], ("one upload answers differently", kind, nm.mismatches(ga, gb), what)
                assert sum(ca) == sum(cb) and (ma is None) == (mb is None), (kind, ca, cb, what)
                if ma is not None:
                    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(ma, mb)), (kind, what)
                assert p.get_option("selection") == (model.selection is not None) and b.get_option("selection") == 0, (kind, what)
        if "merge" in last:
            rec, args = last["merge"]
            if model.n + len(args["G"]) <= nm.em.N_MAX:
                assert _merge(pkg, p, rec, args) == _merge(pkg, b, rec, args), ("merge", what)
                after = model.copy()
                assert after.merge(args["G"], args["C"], rec["radius"])["appended"] == p.num_points - model.n, ("merge", what)
                assert p.num_points == b.num_points == after.n, ("merge", what)
                xa, xb = p.extract_points(), b.extract_points()
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(xa, xb)), ("merged clouds", what)
                es._same_xyz(xa[0], after, np.arange(after.n), ("merged cloud", what))
                assert np.array_equal(xa[1][:, :3], after.rgb), ("merged colours", what)
    finally:
        b.close()


def _run(pkg, orc, family, tag, recs, results, frames_after, rng_seed):
    """Drives the library and the model through recs; results: nearest_model.replay of the sequence (None: the model's
    answers are computed here), tag names the sequence in a failure."""
    model = nm.Model(family)
    p = es._new(pkg, family)
    last, past = {}, []
    try:
        for i, rec in enumerate(recs):
            what = (family, tag, i, {k: v for k, v in rec.items() if k != "state"})
            args = nm.materialize(rec, model, past)
            past.append(args)
            if rec["call"] in ("query", "merge"):
                if results is not None:  # (the references were computed once, for the host tests too)
                    assert results[i][0] == rec and results[i][3] == model.n, what
                    res = results[i][2]
                else:
                    res = nm.apply(model.copy(), rec, args)
                if rec["call"] == "query":
                    _check_query(pkg, p, rec, args, res, model, what)
                else:
                    if res["error"] is None:
                        assert _merge(pkg, p, rec, args) == res["appended"], ("appended", what)
                    else:
                        with pytest.raises(pkg.RtrError) as e:
                            _merge(pkg, p, rec, args)
                        assert e.value.code == pkg._lib.RTR_ERR_UNSUPPORTED, what
                    nm.apply(model, rec, args)
                if res["error"] is None:
                    last[rec.get("kind", "merge")] = (rec, args)
            else:
                _drive(pkg, p, rec, args, model, what)
                nm.apply(model, rec, args)
            es._check_state(pkg, p, model, family, np.random.default_rng([rng_seed, i]), i % 3 == 2, what)
            if i in frames_after:
                es._check_frame(pkg, orc, p, model, i, what)
        es._check_one_upload(pkg, orc, p, model, family, len(recs), (family, tag, len(recs) - 1, "one upload"))
        _check_repeats(pkg, p, model, family, last, (family, tag, "repeats"))
    finally:
        p.close()


@pytest.mark.parametrize("seed", nm.SEEDS)
@pytest.mark.parametrize("family", sorted(nm.FAMILIES))
def test_random_sequence_with_queries_matches_the_model_after_every_step(pkg, orc, family, seed):
    recs = nm.sequence(seed, family, nm.STEPS)
    _run(pkg, orc, family, seed, recs, nm.replay(seed, family, nm.STEPS), set(nm.frame_steps(nm.STEPS)), seed)


# ---- regressions: prefixes of failing random sequences, as literal steps (nearest_model.REGRESSIONS) --------------------
@pytest.mark.parametrize("name", sorted(nm.REGRESSIONS) or [pytest.param(None, marks=pytest.mark.skip(reason="no regression yet"))])
def test_regression_sequences(pkg, orc, name):
    family, recs = nm.REGRESSIONS[name]
    _run(pkg, orc, family, name, recs, None, set(range(len(recs))), 100 + sorted(nm.REGRESSIONS).index(name))
