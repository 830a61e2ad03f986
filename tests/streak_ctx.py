"""Contexts on a torch stream for the tests of overlapped streaks (option "overlap", include/rtr.h): `Scene` (a cloud, its
poses, the oracle's frames), `Ctx` (a context whose frame buffers are aliased as tensors and cloned on the stream between
the renders) and `_exact` (frames against the oracle, bit for bit), shared by test_gpu_overlap_auto.py and
test_gpu_inflight_streak.py.

The plug.  `Ctx.run_plugged` queues a device-side busy wait on the context's stream BEFORE the first render and returns
without synchronising, so its caller makes another library call while every frame of the streak is still queued: the
tail stream is held by the plug, the front stream by the `joined` event the streak's first overlapped frame records on
the tail stream (rtr_api.hip, bin_points).  The caller asserts `not event.query()` directly in front of its call -- a
streak that has already finished has tested nothing.  Anything that allocates inside rtr_render may synchronise the
device, so every plugged streak follows an unplugged one of the same shape in the same context.

The plug is torch.cuda._sleep(cycles); cycles per millisecond are measured once per process with two torch events
(`cycles_per_ms`), never assumed, and checked against a second timed wait before the first use.
Measured on an MI355X: queueing a five-frame streak with its clones takes the host 0.23 - 0.37 ms (MEASURED_QUEUE_MS,
five repetitions at each of 96x64, 208x112 and 640x480, no synchronisation); the spin kernel counts 2.39 M cycles per
millisecond, so PLUG_MS = 60 is 143.5 M cycles, which gave 59.5 - 60.0 ms between two events.  That is 160 x the
queueing time -- the issue asks for 20 x at the least, so that a descheduled host thread does not empty the queue --
and under the cap of 100 ms that keeps a case within seconds.  With the plug set to zero by hand the in-flight
assertions fail (tried once on eight cases, all eight failed): the plug is what holds the queue."""
import numpy as np

# name -> W, H, points, prefilter possible (W % 16 == 0)
SHAPES = {"96x64": (96, 64, 50_000, True), "200x120": (200, 120, 120_000, False), "208x112": (208, 112, 120_000, True),
          "640x480": (640, 480, 300_000, True)}
POSE_IDS = (3, 58, 121, 190, 247, 316, 402, 467, 533)
AUTO = [0, 0, 1, 1, 1, 1, 1, 1, 1]

MEASURED_QUEUE_MS = 0.37  # host time to queue five frames and their clones, no synchronisation (see the module docstring)
PLUG_MS = 60.0


class Scene:
    """A cloud, its poses and the oracle's frames, computed once per module and never changed."""

    def __init__(self, pkg, orc, name, seed=0xC0FFEE10):
        self.pkg, self.orc = pkg, orc
        self.W, self.H, self.n, self.can_filter = SHAPES[name]
        self.xyzw, self.rgba = orc.generate("room_shell", seed, 0, self.n, self.n)
        self.poses = [pkg.orbit_projection(k, self.W, self.H) for k in POSE_IDS]
        self._refs = {}

    def ref(self, P, filtered, cloud=None, tag="base"):
        key = (np.asarray(P, np.float32).tobytes(), bool(filtered), tag)
        if key not in self._refs:
            xyzw, rgba = cloud if cloud is not None else (self.xyzw, self.rgba)
            r = self.orc.project(xyzw, rgba, P, self.W, self.H)
            out = {"depth": r["depth_bits"], "img": r["img"]}
            if filtered:
                f = self.orc.filter(r["depth_bits"], r["img"])
                out = {"depth": f["depth"].view(np.uint32), "img": f["img"], "tensor": f["tensor"], "minmax": f["minmax"]}
            self._refs[key] = out
        return self._refs[key]


_plug = None  # cycles per millisecond, measured once per process


def cycles_per_ms(torch, stream):
    """What one millisecond of torch.cuda._sleep costs in its cycles on this device, from two events on `stream`."""
    def timed(cycles):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            torch.cuda._sleep(int(cycles))
            b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)
    timed(100_000)  # (the kernel's first launch loads its code object)
    rate = 1_000_000 / max(timed(1_000_000), 1e-3)
    return 20.0 * rate / max(timed(20.0 * rate), 1e-3)  # (again over ~20 ms: launch overhead no longer counts)


def plug(torch, stream, ms=None):
    """Queues a busy wait of `ms` (default PLUG_MS) on `stream`; -> the cycles queued.  The first call calibrates."""
    global _plug
    ms = PLUG_MS if ms is None else ms
    if _plug is None:
        rate = cycles_per_ms(torch, stream)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            torch.cuda._sleep(int(rate * 20.0))
            b.record(stream)
        b.synchronize()
        # (it keeps time on the MI355X; where it ever does not, a chain of matrix products has to take its place)
        assert 15.0 <= a.elapsed_time(b) <= 40.0, ("torch.cuda._sleep does not keep time", rate, a.elapsed_time(b))
        _plug = rate
    cycles = int(_plug * ms)
    if cycles > 0:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
    return cycles


class Ctx:
    """A context of its own on a torch stream, with the frame buffers aliased as tensors."""

    def __init__(self, pkg, scene, options=(), upload=True):
        import torch
        self.torch, self.pkg, self.scene = torch, pkg, scene
        self.p = pkg.Projector(0)
        try:
            for k, v in dict(options).items():
                self.p.set_option(k, v)
            if upload:
                self.p.upload_points(scene.xyzw, scene.rgba)
            self.st = torch.cuda.Stream(device=0)
            self.p.set_stream(self.st.cuda_stream)
            self.resolution(scene.W, scene.H)
        except BaseException:
            self.p.close()
            raise

    def resolution(self, W, H):
        L, dev = self.pkg._lib, self.torch.device("cuda", 0)
        self.p.set_resolution(W, H)
        self.bufs = {"depth": self.torch.as_tensor(self.p.device_buffer(L.BUF_DEPTH, "<i4"), device=dev),
                     "img": self.torch.as_tensor(self.p.device_buffer(L.BUF_IMAGE), device=dev),
                     "tensor": self.torch.as_tensor(self.p.device_buffer(L.BUF_TENSOR), device=dev),
                     "minmax": self.torch.as_tensor(self.p.device_buffer(L.BUF_MINMAX, "<i4"), device=dev)}

    def run(self, poses, filtered):
        """Renders the poses back to back; -> overlap_active per frame, the frames (numpy, after one synchronisation)."""
        active, snaps = [], []
        names = ("depth", "img", "tensor", "minmax") if filtered else ("depth", "img")
        for P in poses:
            self.p.render(P, filtered)
            active.append(self.p.get_option("overlap_active"))
            with self.torch.cuda.stream(self.st):
                snaps.append({k: self.bufs[k].clone() for k in names})
        self.st.synchronize()
        frames = []
        for s in snaps:
            f = {k: v.cpu().numpy() for k, v in s.items()}
            f["depth"] = f["depth"].view(np.uint32)
            if filtered:
                f["tensor"] = f["tensor"].view(np.uint16).reshape(5, self.p.H, self.p.W)
                f["minmax"] = f["minmax"].view(np.uint32)
            frames.append(f)
        return active, frames

    def run_plugged(self, poses, filtered):
        """`run` behind a plug (the module docstring) and WITHOUT synchronising: -> overlap_active per frame, a torch
        event recorded behind the last clone, the snapshots (device tensors: `frames` turns them into numpy once the
        event has completed).  filtered: one flag, or one per pose.  `self.first` is an event behind the first frame's
        clones: the device runs a few frames behind the host even unplugged, so the last event alone would still be
        pending for a moment without any plug -- with both pending the WHOLE streak is in flight."""
        flags = [bool(filtered)] * len(poses) if isinstance(filtered, (bool, int)) else [bool(f) for f in filtered]
        active, snaps = [], []
        plug(self.torch, self.st)
        for P, f in zip(poses, flags):
            self.p.render(P, f)
            active.append(self.p.get_option("overlap_active"))
            with self.torch.cuda.stream(self.st):
                snaps.append({k: self.bufs[k].clone() for k in (("depth", "img", "tensor", "minmax") if f else ("depth", "img"))})
            if len(snaps) == 1:  # (behind the FIRST frame: pending as long as nothing of the streak has left the queue)
                self.first = self.torch.cuda.Event()
                self.first.record(self.st)
        event = self.torch.cuda.Event()
        event.record(self.st)
        return active, event, snaps

    @staticmethod
    def frames(event, snaps):
        """The snapshots of run_plugged as run returns them, after waiting for the event."""
        event.synchronize()
        frames = []
        for s in snaps:
            f = {k: v.cpu().numpy() for k, v in s.items()}
            f["depth"] = f["depth"].view(np.uint32)
            if "tensor" in f:
                H, W = f["depth"].shape
                f["tensor"] = f["tensor"].view(np.uint16).reshape(5, H, W)
                f["minmax"] = f["minmax"].view(np.uint32)
            frames.append(f)
        return frames

    def close(self):
        self.p.close()


def _exact(frames, scene, poses, filtered, what, cloud=None, tag="base"):
    for k, (f, P) in enumerate(zip(frames, poses)):
        want = scene.ref(P, filtered, cloud, tag)
        for name, got in f.items():
            w = np.asarray(want[name])
            if name == "tensor":
                w = w.view(np.uint16).reshape(got.shape)
            assert np.array_equal(got.reshape(-1), w.reshape(-1).view(got.dtype)), (what, "frame", k, name,
                                                                                  int((got.reshape(-1) != w.reshape(-1).view(got.dtype)).sum()))
