"""rtr_write_points inside long chains of edits (include/rtr.h section 2f): the seeded sequences of write_model.py --
edit_model's appends, removals, moves, masks, selections and sorts with writes among them (xyz / rgb / both / one
broadcast colour, a random window of a random selection, host or device records) -- on clouds of at most 8192 points,
driven on the library and on the host model.  The checks are test_gpu_edit_sequences.py's own: after EVERY step the
point count, the option read-backs, the keep and selection words and the extraction of every point with indices; after
every fourth step and at the end a filtered frame and its point pass against the oracle; at the end a second context
with one upload of the model's cloud renders the same frames.  In every family a write lands on a cloud that has points
resident behind the written span, a mask in force and -- where the family's options let the library sort a cloud of this
size -- a sorted order: asserted on the step records."""
import numpy as np
import pytest

import edit_model as em
import test_gpu_edit_sequences as es
import write_model as wm

pytestmark = pytest.mark.gpu


def _records(arr, cols, torch_device):
    """The caller's array of a stream: rows padded to `cols` columns, on the host or as a device tensor."""
    if arr is None:
        return None, None
    wide = np.zeros((arr.shape[0], cols), arr.dtype)
    wide[:, :3] = arr
    if torch_device is None:
        return wide, None
    import torch
    t = torch.from_numpy(wide).to(torch_device)
    return t, t


def _drive_write(pkg, p, rec, args, model, what):
    sel = None if rec["sel"] is None else es._arg(pkg, p, rec["form"], rec["sel"], args["bits"])
    k = model.n if args["bits"] is None else int(args["bits"].sum())
    dev = None
    if rec["source"] == "device":
        import torch
        dev = torch.device("cuda", 0)
    if rec["streams"] == "colour":
        got = p.write_points(rgb=args["C"], select=sel, first=args["first"], broadcast=True)
        want = max(0, k - args["first"])
    else:
        X, hold_x = _records(args["X"], 4 if rec["data"] % 2 else 3, dev)
        C, hold_c = _records(args["C"], 4 if rec["data"] % 3 else 3, dev)
        got = p.write_points(X, C, sel, args["first"])
        rows = (args["X"] if args["X"] is not None else args["C"]).shape[0]
        want = min(rows, max(0, k - args["first"]))
    assert got == want, ("points written", got, want, what)


def _run(pkg, orc, family, seed):
    recs = wm.sequence(seed, family, wm.STEPS)
    frames_after = set(wm.frame_steps(wm.STEPS))
    model = wm.Model(family)
    p = es._new(pkg, family)
    try:
        for i, rec in enumerate(recs):
            what = (family, seed, i, {k: v for k, v in rec.items() if k != "state"})
            args = wm.materialize(rec, model)
            if rec["call"] == "write":
                _drive_write(pkg, p, rec, args, model, what)
            else:
                es._drive(pkg, p, rec, args, model, what)
            wm.apply(model, rec, args)
            es._check_state(pkg, p, model, family, np.random.default_rng([seed, i]), i % 3 == 2, what)
            if i in frames_after:
                es._check_frame(pkg, orc, p, model, i, what)
        es._check_one_upload(pkg, orc, p, model, family, len(recs), (family, seed, len(recs) - 1, "one upload"))
    finally:
        p.close()


@pytest.mark.parametrize("seed", wm.SEEDS)
@pytest.mark.parametrize("family", wm.WRITE_FAMILIES)
def test_random_sequence_with_writes_matches_the_model_after_every_step(pkg, orc, family, seed):
    _run(pkg, orc, family, seed)


@pytest.mark.parametrize("family", wm.WRITE_FAMILIES)
def test_a_write_lands_behind_a_mask_in_front_of_resident_points_on_a_sorted_cloud(family):
    """On the step records: some write of the family's sequences changes points while (a) points are resident behind the
    written span, (b) a mask is in force and (c) the cloud was sorted by the library -- (c) where the family can be
    sorted at all: "pack0" runs with auto_reorder = 0 and without point_ids, so nothing ever sorts it."""
    can_sort = em.allows_reorder(family) or em.FAMILIES[family].get("auto_reorder") == 1
    hits = [r["state"] for seed in wm.SEEDS for r in wm.sequence(seed, family, wm.STEPS) if r["call"] == "write"
            and r["state"]["points"] and r["state"]["behind"] and r["state"]["masked"] and (r["state"]["sorted"] or not can_sort)]
    assert hits, family
