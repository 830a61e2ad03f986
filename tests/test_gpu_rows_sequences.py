"""The statistical filter and the normals inside long chains of edits (include/rtr_statistics.h section 6n,
include/rtr_normals.h section 6o): the seeded sequences of rows_model.py -- write_model's appends, removals, moves, masks,
selections, sorts and writes with rtr_select_statistical, rtr_estimate_normals and ProjectCloud.removeStatisticalOutliers
among them, one of the two calls directly behind every edit that rewrites chunk boxes, populations, the permutation or
the upload indices: copies appended beside their originals, the originals removed, copies appended onto a sorted cloud,
a clean-up, one point more and one point fewer -- on clouds of at most 8192 points, driven on the library and on the host
model.  After EVERY such step everything returned equals the model's through rows_model.mismatches (float arrays by
their bits, found, the selection's words and the stats exactly, the moments within statistical_ref.moments_tolerance
with the hits exact against the returned t); an output asked absent is NULL, one asked on the device is a device tensor
read back; and test_gpu_edit_sequences.py's own checks follow (point count, option read-backs, keep and selection words,
the extraction of every point): rtr_estimate_normals leaves the selection alone and creates none,
rtr_select_statistical creates or combines it, the clean-up leaves the model's cloud.  A step the model expects to fail
raises RTR_ERR_UNSUPPORTED and changes nothing, the caller's sentinel-filled arrays included.  Frames and the point pass
are checked after every fourth step and at the end; at the end a second context with one upload of the model's cloud
answers the last successful statistical and normals records as the edited context does, array for array.
test_rows_model_host.py checks the model, the coverage and the sensitivity of exactly these sequences without a GPU."""
import ctypes as C

import numpy as np
import pytest

import rows_model as rm
import test_gpu_edit_sequences as es
import test_gpu_nearest_sequences as ns

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = {"mean": (lambda n: (n,), f32), "found": (lambda n: (n,), np.uint32), "normals": (lambda n: (n, 3), f32),
          "curvature": (lambda n: (n,), f32)}
KEYS = {kind: [kind + "_us0", kind + "_us1", kind + "_us2"] for kind in rm.CALLS}
COUNT_KEYS = {kind: [kind + "_pair_tests_k", kind + "_row_updates_k"] for kind in rm.CALLS}


def _facade(pkg, p):
    """ProjectCloud.removeStatisticalOutliers on the context p (the constructor would make a context of its own and
    upload): the methods themselves on a stub that holds what they use, as test_gpu_nearest_sequences.py runs them."""
    class Stub:
        _p = p
        removeStatisticalOutliers = pkg.ProjectCloud.removeStatisticalOutliers
        removeSelected = pkg.ProjectCloud.removeSelected
        _with_complement = pkg.ProjectCloud._with_complement
    return Stub()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _buffers(rec, n):
    """name -> (the caller's array filled with 7s where the record places it, None where it is absent; its pointer)."""
    out = {}
    for name in rm.ARRAYS[rec["kind"]]:
        shape, dt = SHAPES[name][0](n), SHAPES[name][1]
        where = rec["place"][name]
        if where is None:
            out[name] = (None, None)  # (really NULL)
        elif where == "host":
            a = np.full(shape, 7, dt)
            out[name] = (a, _vp(a))
        else:
            import torch
            t = torch.full(shape, 7, dtype=torch.float32 if dt is f32 else torch.int32, device=torch.device("cuda", 0))
            out[name] = (t, C.c_void_p(t.data_ptr()))
    return out


def _read(a, dt):
    if isinstance(a, np.ndarray):
        return a
    assert a.is_cuda
    return a.cpu().numpy().view(dt)


def _raw(pkg, p, rec, args):
    """The record's call on the C interface -> (return code, the caller's arrays, stats, moments)."""
    L = pkg._lib
    bufs = _buffers(rec, p.num_points)
    st = np.full(4, 77, np.uint64)
    if rec["kind"] == "statistical":
        mom, flags, mul = np.full(3, -1.0), 0, rec["std_mul"]
        if rec["threshold"] is not None:
            mom[2], flags, mul = rec["threshold"], L.STAT_THRESHOLD_GIVEN, 0.0
        code = p._SELECT_OPS[rec["op"]] | (L.SELECT_OUTSIDE if rec["outside"] else 0)
        rc = p._lib.rtr_select_statistical(p._ctx, rec["k"], rec["radius"], mul, flags, code, bufs["mean"][1], bufs["found"][1],
                                           _vp(mom), _vp(st))
        return rc, bufs, st, mom
    view = args["viewpoint"]
    rc = p._lib.rtr_estimate_normals(p._ctx, rec["k"], rec["radius"], 0 if view is None else L.NORMAL_VIEWPOINT, _vp(view),
                                     bufs["normals"][1], bufs["curvature"][1], bufs["found"][1], _vp(st))
    return rc, bufs, st, None


def _returned(pkg, p, rec, bufs, st, mom):
    """rows_model.outputs' dict of what a successful call returned."""
    got = {"stats": tuple(int(v) for v in st)}
    for name, (a, _) in bufs.items():
        if a is not None:
            got[name] = _read(a, SHAPES[name][1])
    if rec["kind"] == "statistical":
        got.update(moments=tuple(float(v) for v in mom), selection=p.download(pkg._lib.BUF_SELECTION))
    return got


def _call(pkg, p, rec, args):
    rc, bufs, st, mom = _raw(pkg, p, rec, args)
    p._chk(rc)
    return _returned(pkg, p, rec, bufs, st, mom)


def _check_rows(pkg, p, rec, args, res, model, what):
    """The record's call on the library against the model's result `res` (model: the state BEFORE the step)."""
    L = pkg._lib
    kind = rec["kind"]
    if kind == "cleanup":
        if res["error"] is not None:
            with pytest.raises(RuntimeError) as e:
                _facade(pkg, p).removeStatisticalOutliers(rec["k"], rec["radius"], rec["std_mul"])
            assert type(e.value) is pkg.RtrError and e.value.code == L.RTR_ERR_UNSUPPORTED, (str(e.value), what)
            return
        got = {"removed": _facade(pkg, p).removeStatisticalOutliers(rec["k"], rec["radius"], rec["std_mul"])}
        assert rm.mismatches(got, rm.outputs(rec, res)) == [], (got, res["removed"], what)
        return
    rc, bufs, st, mom = _raw(pkg, p, rec, args)
    if res["error"] is not None:
        with pytest.raises(RuntimeError) as e:
            p._chk(rc)
        assert type(e.value) is pkg.RtrError and e.value.code == L.RTR_ERR_UNSUPPORTED, (str(e.value), what)
        given = -1.0 if rec.get("threshold") is None else rec["threshold"]
        assert (st == 77).all() and (mom is None or np.array_equal(mom, [-1.0, -1.0, given])), ("stats and moments untouched", what)
        for name, (a, _) in bufs.items():  # (every caller array keeps its sentinel fill)
            assert a is None or (_read(a, SHAPES[name][1]) == 7).all(), (name, "untouched", what)
        return
    p._chk(rc)
    got, want = _returned(pkg, p, rec, bufs, st, mom), rm.outputs(rec, res)
    bad = rm.mismatches(got, want)
    assert bad == [], (bad, got.get("stats"), want.get("stats"), got.get("moments"), want.get("moments"), what)
    for key in KEYS[kind]:
        assert p.get_option(key) > 0, (key, what)
    # (the two counters are kept in thousands, rounded down, and every kept entry was one accepted pair and one row
    # update: they are positive where the model's rows hold a thousand entries; a 37-point cloud may leave them 0)
    if int(res["found"].sum()) >= 1000:
        for key in COUNT_KEYS[kind]:
            assert p.get_option(key) > 0, (key, what)


def _drive(pkg, p, rec, args, model, what):
    if rec["call"] in ("append_near", "append_mirrors"):
        p.append_points(args["xyz"], args["rgb"])
    else:
        ns._drive(pkg, p, rec, args, model, what)


def _identical(a, b):
    return sorted(a) == sorted(b) and all(
        np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32))
        if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


def _check_repeats(pkg, p, model, family, last, what):
    """The last successful statistical and normals records again, on the edited context and on a context that uploads
    the model's cloud once, both without a selection: the same answers, array for array, the moments bit for bit."""
    if model.n == 0:
        return
    b = es._new(pkg, family)
    try:
        b.upload_points(model.xyz, model.rgb)
        for kind in rm.CALLS:
            if kind in last:
                rec, args = last[kind]
                p.clear_selection()
                b.clear_selection()
                if rm.beyond_span(model.xyz, rec["radius"]).any():  # (the cloud has grown past the record's span since: both refuse)
                    for q in (p, b):
                        with pytest.raises(pkg.RtrError) as e:
                            _call(pkg, q, rec, args)
                        assert e.value.code == pkg._lib.RTR_ERR_UNSUPPORTED and q.get_option("selection") == 0, (kind, what)
                    continue
                ga, gb = _call(pkg, p, rec, args), _call(pkg, b, rec, args)
                assert _identical(ga, gb), ("one upload answers differently", kind, [k for k in ga if not _identical({k: ga[k]}, {k: gb[k]})], what)
                assert p.get_option("selection") == b.get_option("selection") == (kind == "statistical"), (kind, what)
    finally:
        b.close()


def _run(pkg, orc, family, tag, recs, results, frames_after, rng_seed):
    """Drives the library and the model through recs; results: rows_model.replay of the sequence (None: the model's
    answers are computed here), tag names the sequence in a failure."""
    model = rm.Model(family)
    p = es._new(pkg, family)
    last, past = {}, []
    try:
        for i, rec in enumerate(recs):
            what = (family, tag, i, {k: v for k, v in rec.items() if k != "state"})
            args = rm.materialize(rec, model, past)
            past.append(args)
            if rec["call"] == "rows":
                if results is not None:  # (the references were computed once, for the host tests too)
                    assert results[i][0] == rec and results[i][3] == model.n, what
                    res = results[i][2]
                else:
                    res = rm.apply(model.copy(), rec, args)
                _check_rows(pkg, p, rec, args, res, model, what)
                rm.advance(model, rec, res)
                if res["error"] is None and rec["kind"] in rm.CALLS:
                    last[rec["kind"]] = (rec, args)
            else:
                _drive(pkg, p, rec, args, model, what)
                rm.apply(model, rec, args)
            es._check_state(pkg, p, model, family, np.random.default_rng([rng_seed, i]), i % 3 == 2, what)
            if i in frames_after:
                es._check_frame(pkg, orc, p, model, i, what)
        es._check_one_upload(pkg, orc, p, model, family, len(recs), (family, tag, len(recs) - 1, "one upload"))
        _check_repeats(pkg, p, model, family, last, (family, tag, "repeats"))
    finally:
        p.close()


@pytest.mark.parametrize("seed", rm.SEEDS)
@pytest.mark.parametrize("family", sorted(rm.FAMILIES))
def test_random_sequence_with_rows_calls_matches_the_model_after_every_step(pkg, orc, family, seed):
    recs = rm.sequence(seed, family, rm.STEPS)
    _run(pkg, orc, family, seed, recs, rm.replay(seed, family, rm.STEPS), set(rm.frame_steps(rm.STEPS)), seed)


# ---- regressions: prefixes of failing random sequences, as literal steps (rows_model.REGRESSIONS) -----------------------
@pytest.mark.parametrize("name", sorted(rm.REGRESSIONS) or [pytest.param(None, marks=pytest.mark.skip(reason="no regression yet"))])
def test_regression_sequences(pkg, orc, name):
    family, recs = rm.REGRESSIONS[name]
    _run(pkg, orc, family, name, recs, None, set(range(len(recs))), 100 + sorted(rm.REGRESSIONS).index(name))
