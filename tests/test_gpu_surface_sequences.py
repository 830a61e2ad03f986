"""The scan registration and the smooth segments inside long chains of edits (include/rtr_register.h section 6p,
include/rtr_segments.h section 6q): the seeded sequences of surface_model.py -- write_model's appends, removals, moves,
masks, selections, sorts and writes with rtr_select_segments, rtr_register_points, ProjectCloud.registerPoints and
ProjectCloud.removeSmallSegments among them, both calls behind every edit that rewrites chunk boxes, populations, the
permutation or the upload indices, and the chains of surface_model._Gen: copies and mirrors beside their originals, the
originals and the copies removed; normals -> segments -> removal -> normals -> segments -> point-to-plane on one pair of
device arrays; an ICP loop on both sides of a move; copies appended onto a sorted cloud; a seeded step on both sides of a
move; winners in the last chunk only, in the first only, nowhere -- on clouds of at most 8192 points, driven on the
library and on the host model.  After EVERY segments or register step, called on the C interface with sentinel-filled
caller arrays, everything asked for equals the model's through surface_model.mismatches, bit for bit (labels in host or
device memory, the selection's words, the stats, the 32 moments and the 12 doubles of the step as uint64); an output not
asked for is NULL; the caller's given points, normals and curvature keep their bits.  The two facade loops run on a stub
and return the model's count, or its pose and rms list, bit for bit.  test_gpu_edit_sequences.py's own checks follow
every step (point count, option read-backs, keep and selection words, the extraction of every point): the registration
leaves the selection alone and creates none, the segments create or combine it, the removal leaves the model's cloud.
A step the model expects to fail raises RTR_ERR_UNSUPPORTED and changes nothing, the caller's sentinel-filled arrays
included.  Frames and the point pass are checked after every fourth step and at the end; at the end a second context
with one upload of the model's cloud answers the last successful record of each call as the edited context does, array
for array.  test_surface_model_host.py checks the model, the coverage and the sensitivity of exactly these sequences
without a GPU."""
import ctypes as C

import numpy as np
import pytest

import surface_model as sm
import test_gpu_edit_sequences as es
import test_gpu_rows_sequences as rs

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
FILL = 0xDEADBEEF


def _facade(pkg, p):
    """ProjectCloud's two loops on the context p (the constructor would make a context of its own and upload): the
    methods themselves on a stub that holds what they use, as test_gpu_nearest_sequences.py runs them."""
    class Stub:
        _p = p
        registerPoints = pkg.ProjectCloud.registerPoints
        selectSegments = pkg.ProjectCloud.selectSegments
        removeSmallSegments = pkg.ProjectCloud.removeSmallSegments
        removeSelected = pkg.ProjectCloud.removeSelected
        _with_complement = pkg.ProjectCloud._with_complement
    return Stub()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _ptr(a):
    """(pointer, the array's bits on the host) of a caller's array: numpy or a device tensor; None stays NULL."""
    if a is None:
        return None, None
    if isinstance(a, np.ndarray):
        return _vp(a), a.view(np.uint32).copy()
    return C.c_void_p(a.data_ptr()), a.cpu().numpy().view(np.uint32).copy()


def _bits(a):
    return a.view(np.uint32) if isinstance(a, np.ndarray) else a.cpu().numpy().view(np.uint32)


def _inputs(p, rec, args, held):
    """The normals and the curvature as the record passes them: (normals, curvature) numpy arrays or device tensors.
    "estimated": what rtr_estimate_normals wrote ON THIS CONTEXT -- the held tensors of the sequence's last normals
    step, or an estimate of this step's own -- never the model's; the model's arrays are compared with them instead."""
    if rec["source"] == "estimated":
        if rec["held"]:
            assert held is not None and held[0].shape[0] == p.num_points, "the pipeline's tensors are there"
            nrm, curv = held
        else:
            nrm, curv, _ = p.estimate_normals(rec["k"], rec["nradius"], device=True)
        assert np.array_equal(_bits(nrm), args["normals"].view(np.uint32)), "rtr_estimate_normals against the model"
        assert np.array_equal(_bits(curv), args["curvature"].view(np.uint32)), "rtr_estimate_normals against the model"
        if rec["where"] == "host":
            nrm, curv = nrm.cpu().numpy(), curv.cpu().numpy()
    else:
        nrm, curv = args["normals"].copy(), None if args["curvature"] is None else args["curvature"].copy()
        if rec["where"] == "device":
            nrm, curv = _dev(nrm), None if curv is None else _dev(curv)
    return nrm, curv


def _rows(rec, G):
    """The given points as the record passes them: rows of 3 or 4 floats, host numpy or a device tensor."""
    rows = np.full((G.shape[0], rec["width"]), 7.5, f32)
    rows[:, :3] = G
    return rows if rec["rows"] == "host" else _dev(rows)


def _segments(pkg, p, rec, args, held):
    """rtr_select_segments on the C interface -> (return code, outputs by name, what must not change)."""
    L, n = pkg._lib, p.num_points
    nrm, curv = _inputs(p, rec, args, held)
    lim = rec["max_curvature"]
    nptr, nbits = _ptr(nrm)
    cptr, cbits = _ptr(curv if lim is not None else None)
    lab = None
    if rec["labels"] == "host":
        lab = np.full(n, FILL, np.uint32)
    elif rec["labels"] == "device":
        lab = _dev(np.full(n, FILL, np.uint32).view(np.int32))
    st = np.full(4, 77, np.uint64) if rec["stats"] else None
    flags = (L.SEGMENT_SEEDED if rec["seeded"] else 0) | (L.SEGMENT_ORIENTED if rec["oriented"] else 0)
    code = p._SELECT_OPS[rec["op"]] | (L.SELECT_OUTSIDE if rec["outside"] else 0)
    rc = p._lib.rtr_select_segments(p._ctx, rec["radius"], rec["cos_angle"], nptr, cptr, 0.0 if lim is None else lim, rec["min_points"],
                                    rec["max_points"], flags, code, _ptr(lab)[0], _vp(st))
    same = np.array_equal(_bits(nrm), nbits) and (cbits is None or np.array_equal(_bits(curv), cbits))
    return rc, {"labels": lab, "stats": st}, same


def _register(pkg, p, rec, args, held):
    """rtr_register_points on the C interface -> (return code, outputs by name, what must not change)."""
    L = pkg._lib
    rows = _rows(rec, args["G"])
    m = args["G"].shape[0]
    gptr, gbits = _ptr(rows)
    nrm, nptr, nbits = None, None, None
    if rec["plane"]:
        nrm, _ = _inputs(p, rec, args, held)
        nptr, nbits = _ptr(nrm)
    pose = None if args["pose"] is None else np.ascontiguousarray(args["pose"], f64).reshape(12)
    before = None if pose is None else pose.copy()
    out = {"moments": np.full(L.REGISTER_MOMENTS, -7.0), "step": np.full(12, -7.0), "stats": np.full(4, 77, np.uint64)}
    out = {k: (v if k in rec["ask"] else None) for k, v in out.items()}
    rc = p._lib.rtr_register_points(p._ctx, gptr if m else None, 4 * rec["width"] if m else 12, m, rec["radius"],
                                    L.REGISTER_POINT_TO_PLANE if rec["plane"] else 0, _vp(pose), nptr, _vp(out["moments"]), _vp(out["step"]),
                                    _vp(out["stats"]))
    same = np.array_equal(_bits(rows), gbits) and (nbits is None or np.array_equal(_bits(nrm), nbits)) and \
        (pose is None or np.array_equal(pose.view(np.uint64), before.view(np.uint64)))
    return rc, out, same


def _untouched(out):
    """Every caller array keeps its sentinel fill."""
    for name, a in out.items():
        if a is None:
            continue
        if name == "labels":
            assert (_bits(a) == FILL).all(), name
        elif name == "stats":
            assert (a == 77).all(), name
        else:
            assert (a == -7.0).all(), name


def _returned(pkg, p, rec, out):
    """surface_model.outputs' dict of what a successful call returned."""
    got = {}
    if out.get("stats") is not None:
        got["stats"] = tuple(int(v) for v in out["stats"])
    if rec["kind"] == "segments":
        got["selection"] = p.download(pkg._lib.BUF_SELECTION)
        if out["labels"] is not None:
            got["labels"] = _bits(out["labels"]).copy()
    else:
        for name in ("moments", "step"):
            if out[name] is not None:
                got[name] = out[name].view(np.uint64).copy()
    return got


def _raw(pkg, p, rec, args, held):
    return (_segments if rec["kind"] == "segments" else _register)(pkg, p, rec, args, held)


def _call(pkg, p, rec, args, held, what=None):
    """A call that is to succeed -> surface_model.outputs' dict of what it returned."""
    rc, out, same = _raw(pkg, p, rec, args, held)
    p._chk(rc)
    assert same, ("the caller's arrays keep their bits", what)
    return _returned(pkg, p, rec, out)


def _loop(pkg, p, rec, args, held):
    nrm = _inputs(p, rec, args, held)[0] if rec["plane"] else None
    pose, rms, st = _facade(pkg, p).registerPoints(_rows(rec, args["G"]), rec["radius"], rec["iterations"], rec["plane"], nrm, args["pose"])
    return {"pose": np.ascontiguousarray(pose, f64).view(np.uint64).reshape(-1), "rms": np.array(rms, f64).view(np.uint64),
            "stats": tuple(int(v) for v in st)}


def _check_surface(pkg, p, rec, args, res, model, held, what):
    """The record's call on the library against the model's result `res` (model: the state BEFORE the step)."""
    L, kind = pkg._lib, rec["kind"]
    if kind in ("remove_small_segments", "register_loop"):
        def run():
            if kind == "register_loop":
                return _loop(pkg, p, rec, args, held)
            return {"removed": _facade(pkg, p).removeSmallSegments(rec["radius"], rec["k"], rec["angle"], rec["max_curvature"], rec["min_points"])}
        if res["error"] is not None:
            with pytest.raises(RuntimeError) as e:
                run()
            assert type(e.value) is pkg.RtrError and e.value.code == L.RTR_ERR_UNSUPPORTED, (str(e.value), what)
            return
        got, want = run(), sm.outputs(rec, res)
        assert sm.mismatches(got, want) == [], (sm.mismatches(got, want), got, want, what)
        return
    if res["error"] is not None:
        if rec["source"] == "estimated" and not rec["held"] and sm.beyond_span(model.xyz, rec["nradius"]).any():
            with pytest.raises(pkg.RtrError) as e:  # (the estimate itself is refused: there are no normals to pass)
                p.estimate_normals(rec["k"], rec["nradius"], device=True)
            assert e.value.code == L.RTR_ERR_UNSUPPORTED, what
            return
        rc, out, same = _raw(pkg, p, rec, args, held)
        with pytest.raises(RuntimeError) as e:
            p._chk(rc)
        assert type(e.value) is pkg.RtrError and e.value.code == L.RTR_ERR_UNSUPPORTED, (str(e.value), what)
        _untouched(out)
        assert same, ("the caller's arrays keep their bits", what)
        return
    # (a registration leaves the selection's bits alone; _check_state shows that it created none)
    sel0 = p.download(L.BUF_SELECTION).copy() if kind == "register" and model.selection is not None else None
    got, want = _call(pkg, p, rec, args, held, what), sm.outputs(rec, res)
    bad = sm.mismatches(got, want)
    assert bad == [], (bad, got.get("stats"), want.get("stats"), what)
    assert sel0 is None or np.array_equal(p.download(L.BUF_SELECTION), sel0), ("register leaves the selection alone", what)


def _normals(pkg, p, rec, args, res, what):
    """A normals step of the pipeline, as test_gpu_rows_sequences.py runs it -> the device tensors it wrote."""
    rc, bufs, st, mom = rs._raw(pkg, p, rec, args)
    if res["error"] is not None:
        with pytest.raises(pkg.RtrError) as e:
            p._chk(rc)
        assert e.value.code == pkg._lib.RTR_ERR_UNSUPPORTED, what
        return None
    p._chk(rc)
    got, want = rs._returned(pkg, p, rec, bufs, st, mom), sm.outputs(rec, res)
    assert sm.rm.mismatches(got, want) == [], (sm.rm.mismatches(got, want), what)
    return bufs["normals"][0], bufs["curvature"][0]


def _check_repeats(pkg, p, model, family, last, what):
    """The last successful segments and register records again, on the edited context and on a context that uploads the
    model's cloud once, both without a selection: the same answers, array for array, and the model's on its final cloud
    (a wrong answer that both contexts share would pass the first comparison).  Where later edits pushed the cloud (or
    the record's own estimate) past the record's span, both refuse it."""
    if model.n == 0:
        return
    b = es._new(pkg, family)
    try:
        b.upload_points(model.xyz, model.rgb)
        for kind in sm.CALLS:
            if kind not in last:
                continue
            rec, args = last[kind]
            rec = dict(rec, held=False)
            args = dict(args)
            p.clear_selection()
            b.clear_selection()
            refused = sm.beyond_span(model.xyz, rec["radius"]).any() if kind == "segments" else False
            if rec.get("source") is not None:  # (the inputs of the cloud as it is now)
                if rec["source"] == "estimated" and sm.beyond_span(model.xyz, rec["nradius"]).any():
                    for q in (p, b):
                        with pytest.raises(pkg.RtrError) as e:
                            q.estimate_normals(rec["k"], rec["nradius"], device=True)
                        assert e.value.code == pkg._lib.RTR_ERR_UNSUPPORTED, (kind, what)
                    continue
                args["normals"], args["curvature"] = model.inputs(rec)
            if refused:
                for q in (p, b):
                    with pytest.raises(pkg.RtrError) as e:
                        _call(pkg, q, rec, args, None)
                    assert e.value.code == pkg._lib.RTR_ERR_UNSUPPORTED and q.get_option("selection") == 0, (kind, what)
                continue
            ga, gb = _call(pkg, p, rec, args, None, what), _call(pkg, b, rec, args, None, what)
            assert sm.mismatches(ga, gb) == [], ("one upload answers differently", kind, sm.mismatches(ga, gb), what)
            bare = model.copy()
            bare.selection = None
            want = sm.outputs(rec, sm.apply(bare, rec, args))
            assert sm.mismatches(ga, want) == [], ("the model on the final cloud", kind, sm.mismatches(ga, want), what)
            assert p.get_option("selection") == b.get_option("selection") == (kind == "segments"), (kind, what)
    finally:
        b.close()


def _run(pkg, orc, family, tag, recs, results, frames_after, rng_seed):
    """Drives the library and the model through recs; results: surface_model.replay of the sequence (None: the model's
    answers are computed here), tag names the sequence in a failure."""
    model = sm.Model(family)
    p = es._new(pkg, family)
    last, past, held = {}, [], None
    try:
        for i, rec in enumerate(recs):
            what = (family, tag, i, {k: v for k, v in rec.items() if k != "state"})
            if results is not None and rec["call"] in ("surface", "rows"):  # (computed once, for the host tests too)
                assert results[i][0] == rec and results[i][3] == model.n, what
                args, res = results[i][1], results[i][2]
            else:
                args = sm.materialize(rec, model, past)
                res = sm.apply(model.copy(), rec, args) if rec["call"] in ("surface", "rows") else None
            past.append(args)
            if rec["call"] == "surface":
                _check_surface(pkg, p, rec, args, res, model, held, what)
                sm.advance(model, rec, res)
                if res["error"] is None and rec["kind"] in sm.CALLS and "ref" not in rec.get("given", {}):
                    last[rec["kind"]] = (rec, args)
            elif rec["call"] == "rows":
                held = _normals(pkg, p, rec, args, res, what)
                sm.advance(model, rec, res)
            else:
                rs._drive(pkg, p, rec, args, model, what)
                sm.apply(model, rec, args)
            es._check_state(pkg, p, model, family, np.random.default_rng([rng_seed, i]), i % 3 == 2, what)
            if i in frames_after:
                es._check_frame(pkg, orc, p, model, i, what)
        es._check_one_upload(pkg, orc, p, model, family, len(recs), (family, tag, len(recs) - 1, "one upload"))
        _check_repeats(pkg, p, model, family, last, (family, tag, "repeats"))
    finally:
        p.close()


@pytest.mark.parametrize("seed", sm.SEEDS)
@pytest.mark.parametrize("family", sorted(sm.FAMILIES))
def test_random_sequence_with_surface_calls_matches_the_model_after_every_step(pkg, orc, family, seed):
    recs = sm.sequence(seed, family, sm.STEPS)
    _run(pkg, orc, family, seed, recs, sm.replay(seed, family, sm.STEPS), set(sm.frame_steps(sm.STEPS)), seed)


# ---- regressions: prefixes of failing random sequences, as literal steps (surface_model.REGRESSIONS) --------------------
@pytest.mark.parametrize("name", sorted(sm.REGRESSIONS) or [pytest.param(None, marks=pytest.mark.skip(reason="no regression yet"))])
def test_regression_sequences(pkg, orc, name):
    family, recs = sm.REGRESSIONS[name]
    _run(pkg, orc, family, name, recs, None, set(range(len(recs))), 100 + sorted(sm.REGRESSIONS).index(name))
