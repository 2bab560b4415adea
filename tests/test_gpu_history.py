"""Every result of a context with a history is the result of a fresh context (history_cases.py has the scenes, the
probes and their inputs; test_history_cases.py checks on the CPU that the inputs can tell the scenes apart).

A history is one `vr.Device(0)` driven through uploads, frames and queries. At each of its check steps every probe of
the current scene runs on it and is compared with the same probe on a fresh context that got the same options, that
one upload and that one probe, and nothing else (`fresh`, computed once per key and shared). Frames, ray grids, record
rows, bitsets, trees, forward queries, ray gradients and profiles have a fixed sum order: they are compared bit for
bit. The three gradients that add doubles with atomics are held to their modules' float64 models within BOUND * S on
either side, and to each other within 2 * BOUND * S. Status codes and the frame's counts are equal.

A history runs step by step: a test asks for one step and pays for the steps before it only if no earlier test has run
them. At most two contexts are alive at a time: the history's and one fresh one.
"""
import ctypes
import functools
import time

import numpy as np
import pytest

import history_cases as H
from helpers import render

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -21  # grad_reference.BOUND = sigma_grad_reference.BOUND (asserted in test_history_cases.py)
DEFAULT = ()
TREES = (("device_bvh", 1), ("half_nodes", 1))


# ------------------------------------------------------------------------------------------------
# contexts and probes
# ------------------------------------------------------------------------------------------------
def new_context(opts=DEFAULT, device=0):
    import torch  # noqa: F401  (first: its HIP runtime is the process runtime)
    import vr_amd as vr
    dev = vr.Device(device)
    for name, value in opts:
        dev.set_option(name, value)
    return dev


def scene_object(name):
    return H.resident_scene() if name == "R" else H.scene(name)


def upload(dev, name):
    dev.upload(scene_object(name), force=True)


def run_probe(dev, name, probe, inp):
    """The probe's arrays, or its status code where the library refuses the call."""
    import vr_amd as vr
    try:
        return H.PROBES[probe](dev, scene_object(name), inp)
    except vr.VRError as e:
        return {"status": np.array([e.status], np.int64)}


def probe_inputs(probe, cur, prev):
    if cur in H.SPHERE_SCENES:
        return H.inputs("B", None)
    return H.inputs(cur, None if probe in H.BATCH_FREE else prev)


FRESH_SECONDS = [0.0, 0]  # time spent in fresh contexts and their number (reported by the last test)


@functools.lru_cache(maxsize=None)
def _fresh(opts, device, name, probe, prev):
    t0 = time.perf_counter()
    dev = new_context(opts, device)
    try:
        upload(dev, name)
        out = run_probe(dev, name, probe, probe_inputs(probe, name, prev))
    finally:
        dev.__del__()
    FRESH_SECONDS[0] += time.perf_counter() - t0
    FRESH_SECONDS[1] += 1
    for a in out.values():
        a.setflags(write=False)
    if "status" not in out and name != "G":
        for key, a in out.items():
            if key.startswith("frame") or key == "rgb":  # a frame that shows nothing compares nothing
                assert np.isfinite(a).all() and a.std() > 0, (name, probe, key)
    return out


def fresh(opts, name, probe, prev, device=0):
    """The probe on a context that got `opts`, the upload of `name` and this probe, and nothing else."""
    return _fresh(opts, device, name, probe, None if probe in H.BATCH_FREE or name in H.SPHERE_SCENES else prev)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare(label, probe, got, want, cur, prev):
    """The mismatches (strings) of one probe's results `got` on a history against `want` on a fresh context."""
    bad = []
    if set(got) != set(want):
        return [f"{label} {probe}: keys {sorted(got)} against {sorted(want)}"]
    for key in want:
        g, w = got[key], want[key]
        if key == "filtered_rays":
            continue  # depends on filter_low by design (history 5 asserts how)
        if (probe, key) in H.ATOMIC_KEYS and H.num_gaussians(cur) > 0:
            G, S = H.gradient_model(probe, cur, prev)
            for side, x in (("history", g), ("fresh", w)):
                err = np.abs(x.astype(np.float64) - G)
                with np.errstate(all="ignore"):
                    rel = float(np.where(S > 0, err / S, 0.0).max())
                print(f"{label} {probe} {side}: max |dev - model| / S = {rel:.3e} (bound {BOUND:.3e})")
                if not (np.isfinite(x).all() and np.all(err <= BOUND * S)):
                    bad.append(f"{label} {probe}.{key} {side}: {rel:.3e} of S from the float64 model (bound {BOUND:.3e})")
            if not np.all(np.abs(g.astype(np.float64) - w) <= 2 * BOUND * S):
                bad.append(f"{label} {probe}.{key}: history and fresh differ by more than 2 BOUND S")
            continue
        if not same_bits(g, w):
            n = int(np.count_nonzero(g != w)) if np.shape(g) == np.shape(w) else -1
            bad.append(f"{label} {probe}.{key}: {n} of {np.size(w)} elements differ "
                       f"({g.tolist() if np.size(g) <= 8 else ''} against {w.tolist() if np.size(w) <= 8 else ''})")
    return bad


def check(dev, opts, cur, prev, probes=None, repeated=False, fresh_opts=None, before=None, device=0, stats_as=None):
    """Runs every probe of `cur` on the history context `dev` and compares it with the fresh context's.

    The five counts of the march probe's frame are those of a fresh context's first frame of the scene, or of its second
    (stats_as "first" / "second"; the default is "second" for a repeated check, else "first"). One bit decides which:
    march_big, which a frame that re-marched 5 % of its pixels switches on for the context's later frames of the scene
    (collect(), vr_frame.cpp). It is on at the frame's start when the context rendered the scene before (repeated), or
    when the frame outgrows the buffers that smaller frames left and is rendered again: its discarded first rendering
    is then that earlier frame. It is off on a new context and where an equal frame of the scene sized the buffers
    before the upload. A scene that never re-marches 5 % has equal first and second counts."""
    label = f"{cur} after {prev}"
    bad = []
    fopts = opts if fresh_opts is None else fresh_opts
    stats_as = stats_as or ("second" if repeated else "first")
    for probe in (H.probes_of(cur) if probes is None else probes):
        if before is not None:
            before()
        t0 = time.perf_counter()
        got = run_probe(dev, cur, probe, probe_inputs(probe, cur, prev))
        t1 = time.perf_counter()
        want = fresh(fopts, cur, probe, prev, device)
        if time.perf_counter() - t0 > 0.25:
            print(f"{label} {probe}: {t1 - t0:.2f} s on the history, {time.perf_counter() - t1:.2f} s for the fresh context")
        if H.is_gaussian(cur) and "status" in want:  # (two equal refusals would compare equal)
            bad.append(f"{label} {probe}: the fresh context answers with status {want['status'].tolist()}")
        if probe == "march" and "stats" in want:
            second = fresh(fopts, cur, "march_second", None, device)
            if not same_bits(second["frame"], want["frame"]):
                bad.append(f"{label}: a fresh context's second march frame is not its first")
            print(f"{label} march counts {got.get('stats', np.zeros(0)).tolist()}: fresh first {want['stats'].tolist()}, "
                  f"second {second['stats'].tolist()}, held to the {stats_as}")
            if stats_as == "second":
                want = dict(want, stats=second["stats"])
        bad += compare(label, probe, got, want, cur, prev)
        check.last[probe] = got
    if cur in H.SPHERE_SCENES:  # the mixture queries refuse a sphere scene, as on a fresh context
        from vr_amd import _lib as L
        for probe in [p for p in H.QUERY_PROBES if p.endswith(".numpy")]:
            got = run_probe(dev, cur, probe, probe_inputs(probe, cur, prev))
            want = fresh(opts, cur, probe, prev, device)
            if not (list(got) == ["status"] and int(got["status"][0]) == L.VR_ERR_UNSUPPORTED and same_bits(got["status"], want["status"])):
                bad.append(f"{label} {probe}: {got} against {want}")
    elif prev is not None and prev != cur and H.is_gaussian(prev) and not repeated and (probes is None or "march" in probes):
        # the two scenes' frames differ, so the previous scene's frame could not pass for this one's
        if same_bits(fresh(opts, cur, "march", None, device)["frame"], fresh(opts, prev, "march", None, device)["frame"]):
            bad.append(f"{label}: the fresh march frames of the two scenes are the same")
    return bad


check.last = {}  # the history side's results of the last check, by probe


def all_queries(dev, name, inp):
    for probe in H.QUERY_PROBES + H.GRADIENT_PROBES:
        run_probe(dev, name, probe, inp)


# ------------------------------------------------------------------------------------------------
# histories: generators of (step, mismatches); the context dies with the generator
# ------------------------------------------------------------------------------------------------
def large_then_small(device=0, probes=None):
    """1 (and 9 on a group). A context that held the large scene renders and answers the small ones in its bytes."""
    import vr_amd as vr
    dev = new_context(DEFAULT, device)
    try:
        upload(dev, "A")
        render(dev, vr.RayMarchingGaussians(H.camera(), env_samples=8), 64, 64)
        render(dev, vr.FreeFlightGaussians(H.camera(), 8), 32, 32)
        if device == 0:
            all_queries(dev, "A", H.warm_inputs("A", 4096))
        for cur, prev in H.SEQUENCES["1-large-then-small"]:
            upload(dev, cur)
            yield f"{cur} after {prev}", check(dev, DEFAULT, cur, prev, probes, device=device)
    finally:
        dev.__del__()


def small_then_large():
    """2. Hints and workspaces sized by 8 x 8 frames and 16-ray queries; then the large scene, and once more with the
    record capacity put back to 4096 before every frame, which outgrows it and is rendered again."""
    import vr_amd as vr
    dev = new_context()
    try:
        upload(dev, "B")
        render(dev, vr.RayMarchingGaussians(H.camera(), env_samples=4), 8, 8)
        render(dev, vr.FreeFlightGaussians(H.camera(), 4), 8, 8)
        render(dev, vr.MultiScatterGaussians(H.camera(), 4), 8, 8, slot=0)
        all_queries(dev, "B", H.warm_inputs("B", 16))
        (cur, prev), = H.SEQUENCES["2-small-then-large"]
        upload(dev, cur)
        # (B's 8 x 8 frames left buffers for a few thousand records: A's frame is rendered again)
        yield "A after B", check(dev, DEFAULT, cur, prev, stats_as="second")
        small = lambda: dev.set_option("record_capacity", 4096)  # noqa: E731
        bad = check(dev, DEFAULT, "A", "B", H.MARCH_PROBES, repeated=True, before=small)
        bad += check(dev, DEFAULT, "A", "B", H.MARCH_PROBES, repeated=True, before=small, fresh_opts=(("record_capacity", 4096),))
        records = int(fresh(DEFAULT, "A", "march", None)["stats"][H.STAT_KEYS.index("scatter_records")])
        if records <= 4096:
            bad.append(f"the march frame has {records} records: it does not outgrow a capacity of 4096")
        yield "A over its record capacity", bad
    finally:
        dev.__del__()


def kinds_lights_environment():
    """3. The volume type flips four times, the light count and the environment colour change."""
    dev = new_context()
    try:
        before = None
        for cur, prev in H.SEQUENCES["3-kinds-lights-environment"]:
            upload(dev, cur)
            # (A's frame outgrows the buffers that B's left: rendered again)
            yield f"{cur} after {before}", check(dev, DEFAULT, cur, prev, stats_as="second" if cur == "Aenv" else None)
            before = cur
    finally:
        dev.__del__()


def trees():
    """4. Device-built trees: with and without a tight tree, without half nodes, from resident tensors."""
    dev = new_context(TREES)
    try:
        for cur, prev in H.SEQUENCES["4-trees"]:
            upload(dev, cur)
            # (a new context's first frame sizes its buffers, and A's frames left room for every later scene and for A again)
            yield f"{cur} after {prev}", check(dev, TREES, cur, prev)
    finally:
        dev.__del__()


def heuristic_state():
    """5. march_big, the list filter's self-switch and the inline shadow rays: per-scene picks made from frames."""
    import vr_amd as vr
    dev = new_context()
    try:
        (f, _), (b, f_), (a, b_), (c, a_), (a2, c_) = H.SEQUENCES["5-heuristic-state"]
        upload(dev, f)
        for k in range(3):
            yield f"F, check {k + 1}", check(dev, DEFAULT, f, None, repeated=k > 0)
        upload(dev, b)
        yield "B after F", check(dev, DEFAULT, b, f_)
        upload(dev, a)
        for k in range(4):
            # (check 1: A's frame outgrows the buffers that F's and B's frames left and is rendered again)
            bad = check(dev, DEFAULT, a, b_, repeated=k > 0, stats_as="second")
            # The list filter: a fresh context's t_eps frame runs it and cuts under a third of the environment rays, so
            # a context leaves it out from its second frame of the scene on: here the t_eps frame follows the t_eps 0
            # frame in every check. The frames are the same bits either way (compared above).
            cut, rays = (int(v) for v in fresh(DEFAULT, "A", "march_eps", None)["filtered_rays"])
            now = int(check.last["march_eps"]["filtered_rays"][0])
            print(f"A: a fresh context's t_eps frame cuts {cut} of {rays} environment rays, check {k + 1} cuts {now}")
            if not 0 < 3 * cut < rays:
                bad.append(f"a fresh context cuts {cut} of {rays} environment rays: not in (0, a third)")
            if now != 0:
                bad.append(f"check {k + 1}: the t_eps frame cut {now} rays, the filter should be left out")
            yield f"A after B, check {k + 1}", bad
        dev.set_option("ff_nee_queue", 1)  # a queue of one ray per path fills: rendered again, then inline
        got = run_probe(dev, "A", "multi", H.inputs("A", None))
        bad = compare("A, ff_nee_queue 1", "multi", got, fresh(DEFAULT, "A", "multi", None), "A", None)
        # The instrumented render counts the shadow rays traced inline and queued: this context queues none any more, a
        # new one with the default queue queues some (its paths scatter more than once: test_history_cases.py).
        integ = vr.MultiScatterGaussians(H.camera(), 4)
        now = dev.count_work(integ.camera, integ.params, 24, 24)["path"]
        ref = new_context()
        try:
            upload(ref, "A")
            new = ref.count_work(integ.camera, integ.params, 24, 24)["path"]
        finally:
            ref.__del__()
        print(f"shadow rays inline / queued: {now['nee_inline']} / {now['nee_queued']} after the queue of 1 filled, "
              f"{new['nee_inline']} / {new['nee_queued']} on a new context, {new['paths']} paths")
        if not (now["nee_queued"] == 0 and now["nee_inline"] > 0 and new["nee_queued"] > new["paths"]):
            bad.append(f"the context does not trace inline, or a new one queues at most a ray per path: {now} against {new}")
        if now["nee_inline"] + now["nee_queued"] != new["nee_inline"] + new["nee_queued"]:
            bad.append(f"the two contexts trace other numbers of shadow rays: {now} against {new}")
        yield "A with a shadow-ray queue of 1", bad
        upload(dev, c)
        queue1 = (("ff_nee_queue", 1),)
        bad = check(dev, queue1, c, a_, H.FREE_FLIGHT_PROBES)
        bad += check(dev, queue1, c, a_, H.FREE_FLIGHT_PROBES, fresh_opts=DEFAULT)  # (the queue's size changes no frame)
        yield "C after A, free flight", bad
        dev.set_option("ff_nee_queue", 6)
        upload(dev, a2)
        # (A's own earlier frames sized every buffer: nothing is rendered again, march_big starts off)
        yield "A after C", check(dev, DEFAULT, a2, c_)
    finally:
        dev.__del__()


def tables():
    """6. Step tables keyed by step size that regrow and never shrink, and the PCG jump table."""
    import vr_amd as vr
    dev = new_context()
    try:
        (cur, _), = H.SEQUENCES["6-tables"]
        assert cur == "B"
        upload(dev, "B")
        run_probe(dev, "B", "march", H.inputs("B", None))  # a short table first
        yield "far camera after the main one", check(dev, DEFAULT, "B", None, ("march_far",))
        yield "main camera after the far one", check(dev, DEFAULT, "B", None, H.MARCH_PROBES)
        render(dev, vr.RayMarchingGaussians(H.camera(), env_samples=37), 32, 32)
        yield "4 environment samples after 37", check(dev, DEFAULT, "B", None, H.MARCH_PROBES, repeated=True)
        render(dev, vr.RayMarchingGaussians(H.camera(), step_size=0.02, env_samples=4), 32, 32)
        render(dev, vr.PureRayMarching(H.camera(), step_size=0.02, env_samples=4), 24, 24)
        yield "step 0.01 after 0.02", check(dev, DEFAULT, "B", None, H.MARCH_PROBES, repeated=True)
    finally:
        dev.__del__()


# Every option of kOptions (vr_device.cpp) with a non-default value; True: it applies at the next upload (vr_hip.h)
OPTION_ROUND_TRIP = (("half_nodes", 0, True), ("secondary_budget", 0, False), ("ff_window0", 2, False), ("ff_nee_queue", 16, False),
                     ("device_bvh", 1, True), ("march_binned", 1, False), ("ff_solver", 1, False), ("start_subtree", 0, False),
                     ("ff_kernel", 1, False), ("sec_tight", 0, True), ("march_wide_min", 0, False), ("sec_filter", 0, False),
                     ("record_capacity", 4096, False))


def option_round_trip():
    """7. Every option set to a non-default value, used, and restored."""
    import vr_amd as vr
    dev = new_context()
    try:
        bad = []
        if sorted(n for n, _, _ in OPTION_ROUND_TRIP) != sorted(vr.Device.OPTIONS):
            bad.append("OPTION_ROUND_TRIP does not name every option")
        upload(dev, "A")
        inp = H.warm_inputs("A", 64)
        for name, value, at_upload in OPTION_ROUND_TRIP:
            saved = dev.get_option(name)
            dev.set_option(name, value)
            if at_upload:
                upload(dev, "A")
            if name.startswith("ff_"):
                render(dev, vr.FreeFlightGaussians(H.camera(), 2), 16, 16)
            else:
                render(dev, vr.RayMarchingGaussians(H.camera(), env_samples=4, t_eps=1e-3), 16, 16)
            run_probe(dev, "A", "transmittance.numpy", inp)
            dev.set_option(name, saved)
            upload(dev, "A")
        # (the 16 x 16 frames left buffers for a quarter of the 32 x 32 frame's records: it is rendered again)
        (cur, prev), = H.SEQUENCES["7-option-round-trip"]
        yield "A after every option's round trip", bad + check(dev, DEFAULT, cur, prev, stats_as="second")
    finally:
        dev.__del__()


def sfd_answer(dev, n):
    """vr_sfd_loss_diff of seeded losses over the 24 x 24 recordings of slots 0 and 1: the sums, or the status."""
    import vr_amd as vr
    from vr_amd import _lib as L
    rng = np.random.default_rng(5)
    lb, lp = rng.uniform(0, 1, 24 * 24).astype(np.float32), rng.uniform(0, 1, 24 * 24).astype(np.float32)
    out = np.zeros(max(n, 1), np.float64)
    try:
        L.check(L.lib().vr_sfd_loss_diff(dev._h, L.fptr(lb), L.fptr(lp), 24, 24, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n))
    except vr.VRError as e:
        return {"status": np.array([e.status], np.int64)}
    return {"sums": out[:n]}


def queries_between_frames():
    """8. Frames and queries interleaved in two orders; what an upload does to a pending event count and to recordings."""
    import torch
    import vr_amd as vr
    from vr_amd import _lib as L
    dev = new_context()
    try:
        upload(dev, "A")
        frames, queries = list(("tree",) + H.FRAME_PROBES), list(H.QUERY_PROBES + H.GRADIENT_PROBES)
        mixed = [p for k, q in enumerate(queries) for p in [q] + frames[k:k + 1]]  # a query, a frame, a query, ...
        (cur, prev), = H.SEQUENCES["8-queries-between-frames"]
        assert (cur, prev) == ("A", None)
        # (the march frame is the new context's first frame: queries and the tree read-back come before it)
        yield "queries before frames, interleaved", check(dev, DEFAULT, "A", None, mixed, stats_as="first")
        yield "frames before queries, reversed", check(dev, DEFAULT, "A", None, list(reversed(mixed)), repeated=True)
        # a count of A's events does not license a fill after B's upload
        inp = H.inputs("A", None)
        o, d = torch.from_numpy(np.array(inp.o)).cuda(), torch.from_numpy(np.array(inp.d)).cuda()
        rays, stream = dev._pack_rays_torch(o, d, 0.0)
        off = torch.zeros(inp.n + 1, dtype=torch.int32, device="cuda")
        total = ctypes.c_uint64()
        L.check(L.lib().vr_query_events_count_device(dev._h, rays.data_ptr(), inp.n, off.data_ptr(), ctypes.byref(total)))
        bad = [] if total.value > 0 else ["A's rays meet no event"]
        upload(dev, "B")
        t = torch.empty(total.value, dtype=torch.float32, device="cuda")
        ev = torch.empty(total.value, dtype=torch.int32, device="cuda")
        st = L.lib().vr_query_events_fill_device(dev._h, rays.data_ptr(), inp.n, off.data_ptr(), t.data_ptr(), ev.data_ptr(), total.value, stream)
        torch.cuda.synchronize()
        if st != L.VR_ERR_INVALID:
            bad.append(f"vr_query_events_fill_device after an upload returned {st}, not VR_ERR_INVALID")
        yield "event count across an upload", bad
        # vr_sfd_loss_diff's contract (vr_device.cpp): slots 0 and 1 hold recordings of this frame size and of n Gaussians.
        # The recordings are the context's, not the scene's: they outlive an upload, and the sums over them are what a
        # context gives that recorded the same and uploaded nothing; any other n is refused.
        upload(dev, "A")
        run_probe(dev, "A", "multi", inp)
        upload(dev, "B")
        got = sfd_answer(dev, H.num_gaussians("A"))
        ref = new_context()
        try:
            upload(ref, "A")
            run_probe(ref, "A", "multi", inp)
            want = sfd_answer(ref, H.num_gaussians("A"))
        finally:
            ref.__del__()
        bad = compare("recordings of A after B's upload", "sfd", got, want, "A", None)
        if "sums" not in want or not np.any(want["sums"] != 0):
            bad.append(f"the fresh context's sums say nothing: {want}")
        other = sfd_answer(dev, H.num_gaussians("B"))
        if list(other) != ["status"] or int(other["status"][0]) != L.VR_ERR_INVALID:
            bad.append(f"vr_sfd_loss_diff with B's n on A's recordings: {other}")
        yield "recordings across an upload", bad
    finally:
        dev.__del__()


def two_rank_group():
    """9. History 1's steps on a two-rank group of one GPU, against a fresh group and a fresh single context."""
    gen = large_then_small((0, 0), H.GROUP_PROBES)
    try:
        for step, bad in gen:
            cur = step.split()[0]
            for probe in H.GROUP_PROBES:  # frames of a group and of one device are bit-equal
                bad += compare(f"{step}, group against one device", probe, fresh(DEFAULT, cur, probe, None, (0, 0)),
                               fresh(DEFAULT, cur, probe, None, 0), cur, None)
            yield step, bad
    finally:
        gen.close()


HISTORIES = {
    "1-large-then-small": (large_then_small, ("B after A", "G after B", "B after G")),
    "2-small-then-large": (small_then_large, ("A after B", "A over its record capacity")),
    "3-kinds-lights-environment": (kinds_lights_environment, ("S2 after None", "B after S2", "S3 after B", "Aenv after S3", "S2 after Aenv")),
    "4-trees": (trees, ("A after None", "D after A", "E after D", "R after E", "A after R")),
    "5-heuristic-state": (heuristic_state, ("F, check 1", "F, check 2", "F, check 3", "B after F", "A after B, check 1",
                                            "A after B, check 2", "A after B, check 3", "A after B, check 4",
                                            "A with a shadow-ray queue of 1", "C after A, free flight", "A after C")),
    "6-tables": (tables, ("far camera after the main one", "main camera after the far one", "4 environment samples after 37",
                          "step 0.01 after 0.02")),
    "7-option-round-trip": (option_round_trip, ("A after every option's round trip",)),
    "8-queries-between-frames": (queries_between_frames, ("queries before frames, interleaved", "frames before queries, reversed",
                                                          "event count across an upload", "recordings across an upload")),
    "9-two-rank-group": (two_rank_group, ("B after A", "G after B", "B after G")),
}


class Runner:
    """The one history that is under way: its generator and the results of the steps it has reached."""
    name, gen, results, error = None, None, {}, None

    @classmethod
    def result(cls, name, step):
        if cls.name != name:
            cls.stop()
            cls.name, cls.gen, cls.results, cls.error = name, HISTORIES[name][0](), {}, None
        while step not in cls.results:
            if cls.error is not None:  # the history ended in an exception: its later steps fail with it, at once
                raise AssertionError(f"history {name} ended before step {step!r}: {cls.error}")
            try:
                got, bad = next(cls.gen)
            except BaseException as e:
                cls.gen, cls.error = None, repr(e)
                raise
            cls.results[got] = bad
        if list(cls.results) == list(HISTORIES[name][1]):
            cls.stop(keep=True)
        return cls.results[step]

    @classmethod
    def stop(cls, keep=False):
        if cls.gen is not None:
            cls.gen.close()  # (its context is destroyed)
        cls.gen = None
        if not keep:
            cls.name, cls.results, cls.error = None, {}, None


FRESH_PARTS = {"march": ("tree", "march", "march_eps", "spheres", "hitmask"), "second": ("march_second",), "frames": ("pure", "freeflight", "multi"),
               "batch": ("raygrid",) + H.QUERY_PROBES + H.GRADIENT_PROBES}


FRESH_CASES = [(name, part) for name in H.GAUSSIAN_SCENES + H.SPHERE_SCENES for part in FRESH_PARTS
               if set(H.probes_of(name) + (("march_second",) if H.is_gaussian(name) else ())) & set(FRESH_PARTS[part])]


@pytest.mark.parametrize("name,part", FRESH_CASES, ids=[f"{n}-{p}" for n, p in FRESH_CASES])
def test_fresh_contexts_show_their_scene(name, part):
    """The fresh side of a scene's probes on its own batch, one context each (`fresh` asserts that a frame is finite and
    not flat); the histories below compare against these. The empty scene's frame is its environment colour."""
    for probe in H.probes_of(name) + (("march_second",) if H.is_gaussian(name) else ()):
        if probe in FRESH_PARTS[part]:
            out = fresh(DEFAULT, name, probe, None)
            assert "status" not in out, (probe, out)
    if name == "G" and part == "march":
        assert np.array_equal(fresh(DEFAULT, "G", "march", None)["frame"], np.broadcast_to(H.scene("G").env_color, (32, 32, 3)))


STEPS = [(name, step) for name, (_, steps) in HISTORIES.items() for step in steps]


@pytest.mark.parametrize("name,step", STEPS, ids=[f"{n}:{s.replace(' ', '_')}" for n, s in STEPS])
def test_history(name, step):
    bad = Runner.result(name, step)
    assert not bad, "\n".join(bad)


def test_no_context_is_left_alive():
    """The last history's context is destroyed, and the cost of the fresh contexts is reported."""
    Runner.stop()
    assert Runner.gen is None
    print(f"fresh contexts: {FRESH_SECONDS[1]} in {FRESH_SECONDS[0]:.1f} s")
