"""The analysis calls inside long chains of edits (include/rtr.h sections 6g - 6k): the seeded sequences of
analysis_model.py -- write_model's appends, removals, moves, masks, selections, sorts and writes with
rtr_select_voxel_grid, rtr_select_neighbours, rtr_select_clusters, rtr_select_near, rtr_count_in_bands and rtr_fit_plane
among them, a step of those directly behind every edit that rewrites chunk boxes, populations or the permutation -- on
clouds of at most 8192 points, driven on the library and on the host model.  After EVERY analysis step the returned
statistics, labels, near bits, band counts and the plane equal the model's exactly; then come test_gpu_edit_sequences.py's
own checks (point count, option read-backs, keep and selection words, the extraction of every point), so a call that
must leave the selection alone is seen to.  A call the model expects to fail raises the facade's exception and changes
nothing.  Frames and the point pass are checked after every fourth step and at the end; at the end a second context with
one upload of the model's cloud renders the same frames and answers the last successful analysis step of every kind as
the edited context does.  test_analysis_model_host.py checks the model, the coverage and the sensitivity of exactly
these sequences without a GPU."""
import numpy as np
import pytest

import analysis_model as am
import test_gpu_edit_sequences as es
import test_gpu_write_sequences as ws

pytestmark = pytest.mark.gpu


def _given(rec, G):
    """The given points as the record passes them: rows of 3 or 4 floats, host numpy or a device tensor."""
    rows = np.full((G.shape[0], rec["width"]), 7.5, np.float32)
    rows[:, :3] = G
    if rec["source"] == "host":
        return rows
    import torch
    return torch.from_numpy(rows).to(torch.device("cuda", 0))


def _call(pkg, p, rec, args):
    """The record's call on the facade -> a dict of everything it returned."""
    kind, kw = rec["kind"], {"op": rec["op"], "outside": rec["outside"]}
    if kind == "voxel":
        return {"stats": p.select_voxel_grid(rec["cell"], rec["origin"], rec["min_count"], **kw)}
    if kind == "neighbours":
        return {"stats": p.select_neighbours(rec["radius"], rec["min_neighbours"], **kw)}
    if kind == "clusters":
        st, lab = p.select_clusters(rec["radius"], rec["min_points"], rec["max_points"], seeded=rec["seeded"], labels=True, **kw)
        return {"stats": st, "labels": lab}
    if kind == "near":
        out = p.select_near(_given(rec, args["G"]), rec["radius"], near=rec["near"], given_only=rec["given_only"], **kw)
        got = {"stats": out[0], "near": out[1]} if rec["near"] or rec["given_only"] else {"stats": out}
        got["chunks"] = (p.get_option("near_chunks_skipped"), p.get_option("near_chunks_decoded"))
        return got
    if kind == "bands":
        counts, st = p.count_in_bands(args["bands"], selected=rec["selected"])
        return {"counts": counts, "stats": st}
    if kind == "fit_plane":
        plane, inliers, st = p.fit_plane(rec["dist"], rec["iterations"], rec["seed"], selected=rec["selected"])
        return {"plane": plane, "inliers": inliers, "stats": st}
    raise ValueError(kind)


def _outcome(pkg, p, rec, args):
    """_call, or ("error", exception type, code) of the exception it raised."""
    try:
        return _call(pkg, p, rec, args)
    except pkg.RtrError as e:
        return ("error", "RtrError", e.code)
    except RuntimeError:
        return ("error", "RuntimeError", None)


def _same(a, b):
    if isinstance(a, tuple) or isinstance(b, tuple):
        return a == b
    if set(a) != set(b):
        return False
    for k in a:
        x, y = a[k], b[k]
        if k == "chunks":  # (the split between skipped and decoded chunks depends on the resident order)
            if sum(x) != sum(y):
                return False
        elif k == "stats" and len(x) == 4 and "counts" in a:  # (so does the split of the (chunk, band) pairs)
            if x[0] != y[0] or sum(x[1:]) != sum(y[1:]):
                return False
        elif isinstance(x, np.ndarray):
            if not np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y):
                return False
        elif x != y:
            return False
    return True


def _drive_analysis(pkg, p, rec, args, res, model, what):
    """The record's call on the library against the model's result `res` (model: the state BEFORE the step)."""
    kind, n = rec["kind"], model.n
    chunks = (n + 255) // 256
    if res["error"] is not None:
        with pytest.raises(RuntimeError) as e:
            _call(pkg, p, rec, args)
        if res["error"] == "unsupported":
            assert type(e.value) is pkg.RtrError and e.value.code == pkg._lib.RTR_ERR_UNSUPPORTED, (str(e.value), what)
        else:  # (fit_plane: every candidate was degenerate -- the library call succeeds, the facade raises)
            assert type(e.value) is RuntimeError, (repr(e.value), what)
        return
    got = _call(pkg, p, rec, args)
    st = got["stats"]
    if kind == "bands":
        assert st[0] == res["stats"][0], ("population", st, res["stats"], what)
        assert st[1] + st[2] + st[3] == chunks * len(rec["bands"]), ("(chunk, band) pairs", st, what)
        assert got["counts"].dtype == np.uint64 and np.array_equal(got["counts"], res["counts"]), ("band counts", what)
    elif kind == "fit_plane":
        assert st == tuple(int(v) for v in res["stats"]), ("stats", st, res["stats"], what)
        assert got["inliers"] == res["stats"][0], ("inliers", what)
        assert np.array_equal(got["plane"].view(np.uint32), res["plane"].view(np.uint32)), ("plane", got["plane"], res["plane"], what)
    else:
        assert st == tuple(int(v) for v in res["stats"]), ("stats", st, res["stats"], what)
    if kind == "clusters":
        assert got["labels"].dtype == np.uint32 and np.array_equal(got["labels"], res["labels"]), ("labels", what)
    if kind == "near":
        assert got["chunks"][0] + got["chunks"][1] == chunks, ("near_chunks_skipped + near_chunks_decoded", got["chunks"], what)
        assert ("near" in got) == (res["near"] is not None)
        if res["near"] is not None:
            assert got["near"].shape == res["near"].shape and np.array_equal(got["near"], res["near"]), ("near bits", what)


def _check_repeats(pkg, p, model, family, last, what):
    """The last successful analysis step of every kind again, on the edited context and on a context that uploads the
    model's cloud once: the same answers.  Both start without a selection and run the kinds in one order, so each step
    meets the selection the steps before it left in its own context."""
    if model.n == 0 or not last:
        return
    b = es._new(pkg, family)
    try:
        b.upload_points(model.xyz, model.rgb)
        if model.keep is not None:
            b.set_point_keep(model.keep)
        p.clear_selection()
        for kind in am.KINDS:
            if kind not in last:
                continue
            rec, args = last[kind]
            ga, gb = _outcome(pkg, p, rec, args), _outcome(pkg, b, rec, args)
            assert _same(ga, gb), ("one upload answers differently", kind, ga, gb, what)
            assert p.get_option("selection") == b.get_option("selection"), (kind, what)
            if p.get_option("selection"):
                L = pkg._lib
                assert np.array_equal(p.download(L.BUF_SELECTION), b.download(L.BUF_SELECTION)), ("selection words", kind, what)
        p.clear_selection()
    finally:
        b.close()


def _run(pkg, orc, family, tag, recs, results, frames_after, rng_seed):
    """Drives the library and the model through recs; results: analysis_model.replay of the sequence (None: the model's
    analysis results are computed here), tag names the sequence in a failure."""
    model = am.Model(family)
    p = es._new(pkg, family)
    last = {}
    try:
        for i, rec in enumerate(recs):
            what = (family, tag, i, {k: v for k, v in rec.items() if k not in ("state", "bands")})
            args = am.materialize(rec, model)
            if rec["call"] == "analysis":
                if results is not None:  # (the references were computed once, for the host tests too)
                    res, after = results[i][2], results[i][5]
                    assert results[i][0] == rec and results[i][3] == model.n, what
                    _drive_analysis(pkg, p, rec, args, res, model, what)
                    model.selection = None if after is None else after.copy()
                else:
                    before = model.copy()
                    res = am.apply(model, rec, args)
                    _drive_analysis(pkg, p, rec, args, res, before, what)
                if res["error"] is None:
                    last[rec["kind"]] = (rec, args)
            elif rec["call"] == "write":
                ws._drive_write(pkg, p, rec, args, model, what)
                am.apply(model, rec, args)
            else:
                es._drive(pkg, p, rec, args, model, what)
                am.apply(model, rec, args)
            es._check_state(pkg, p, model, family, np.random.default_rng([rng_seed, i]), i % 3 == 2, what)
            if i in frames_after:
                es._check_frame(pkg, orc, p, model, i, what)
        es._check_one_upload(pkg, orc, p, model, family, len(recs), (family, tag, len(recs) - 1, "one upload"))
        _check_repeats(pkg, p, model, family, last, (family, tag, "repeats"))
        model.selection = None
        es._check_state(pkg, p, model, family, np.random.default_rng([rng_seed, len(recs)]), True, (family, tag, "after the repeats"))
    finally:
        p.close()


@pytest.mark.parametrize("seed", am.SEEDS)
@pytest.mark.parametrize("family", sorted(am.FAMILIES))
def test_random_sequence_with_analysis_matches_the_model_after_every_step(pkg, orc, family, seed):
    recs = am.sequence(seed, family, am.STEPS)
    _run(pkg, orc, family, seed, recs, am.replay(seed, family, am.STEPS), set(am.frame_steps(am.STEPS)), seed)


# ---- regressions: prefixes of failing random sequences, as literal steps (analysis_model.REGRESSIONS) -------------------
@pytest.mark.parametrize("name", sorted(am.REGRESSIONS) or [pytest.param(None, marks=pytest.mark.skip(reason="no regression yet"))])
def test_regression_sequences(pkg, orc, name):
    family, recs = am.REGRESSIONS[name]
    _run(pkg, orc, family, name, recs, None, set(range(len(recs))), 100 + sorted(am.REGRESSIONS).index(name))
