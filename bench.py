#!/usr/bin/env python
"""bench.py — frames/s of the MI355X-native ElasticFusion per-frame hot path.

    python bench.py --gpus 1 --steps 200 --warmup 20
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one ef_process_frame_dev() over one 640x480 synthetic RGB-D frame (BASELINE.json configs[1] shape:
640x480 replay, full 3-level ICP + photometric + SO(3) tracking, surfel fuse / clean / predict) with the frames
already resident in HBM.  N > 1: rank r replays its own independent sequence (seed 0xEF0001 + r) on GPU r
("replicas only", no data-path collective); RCCL is used once to gather the per-rank stats.
Prints ONE JSON line on rank 0.

A plain run sets up, pre-rolls and warms up, times --steps frames and prints the line.  Everything else it can measure (per-frame
times and rooflines on the frames behind the timed region, `value_200_steps`, the box calibration, the side legs, the CPU baseline and
the ATE against it) runs only with --full:

    python bench.py --gpus 1 --steps 200 --warmup 20 --full

--dump-outputs DIR writes what the timed path computed in its last step (pose, surfel map) as DIR/<name>.npy.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s achievable
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC for RCCL ranks; must be set before the HIP runtime starts
W, H = 640, 480                # default workload = BASELINE.json configs[1] shape; --width/--height select configs[2] (1280x960)


def _gen_frame(args):
    seed, k, w, h = args
    from elasticfusion_amd import synth
    rgb, depth, T = _gen_frame.cache.setdefault((seed, w, h), synth.Sequence(seed, width=w, height=h)).frame(k)
    return rgb, depth, T


_gen_frame.cache = {}


PROBE_FRAMES = 24   # frames AFTER the timed region on which the two roofline kernels are sampled (see main)
SELF_CHECK = 200    # frames behind the probe frames, timed as ONE more region on the default N = 1 line (`value_200_steps`): the driver's command times 20 steps
                    # (~12 ms), where +-3 % of run-to-run noise decides every comparison; the longer region of the same run shows it in the record itself
PREROLL = 100   # untimed frames before --warmup: the map reaches its steady state (stable surfels, model-fed tracker, clean() removing
               # stale unstable surfels) whatever --steps / --warmup the caller chose, so the timed region is the representative workload
DISTINCT_FRAMES = 512   # at most this many frames are rendered (~0.3 s of host time each); a longer replay runs back and forth over them
DUMP_BYTES = 64 << 20   # --dump-outputs: the budget of all files together


def frame_index(k: int, n_distinct: int) -> int:
    """frame of the sequence shown at replay step k: 0, 1, .., n_distinct - 1, n_distinct - 2, .., 1, 0, 1, ..  (the camera turns round
    at either end, so consecutive steps stay one frame's motion apart); the identity while k < n_distinct"""
    if n_distinct < 2:
        return 0
    p = k % (2 * n_distinct - 2)
    return p if p < n_distinct else 2 * n_distinct - 2 - p


def replay_frames(seed: int, n: int, w: int = W, h: int = H, ranks_on_host: int = 1, cache: str | None = None):
    """the n frames of a replay: the first min(n, DISTINCT_FRAMES) frames of the sequence, then back and forth over them (frame_index).
    The list holds references, so a frame rendered once is also uploaded once (see upload_frames)."""
    nd = min(n, DISTINCT_FRAMES)
    path = f"{cache}.{w}x{h}.{nd}.npz" if cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        distinct = [(z["rgb"][k], z["depth"][k], z["T"][k]) for k in range(nd)]
    else:
        distinct = generate_frames(seed, nd, w, h, ranks_on_host)
        if path:
            np.savez(path, rgb=np.stack([f[0] for f in distinct]), depth=np.stack([f[1] for f in distinct]), T=np.stack([f[2] for f in distinct]))
    return [distinct[frame_index(k, nd)] for k in range(n)]


def upload_frames(api, frames):
    """device copies of a replay's frames, one per distinct frame object"""
    up = {}
    for r, d, _ in frames:
        if id(r) not in up:
            up[id(r)] = (api.DevBuf.from_array(r), api.DevBuf.from_array(d))
    return [up[id(r)] for r, _, _ in frames]


def dump_outputs(ef, out_dir):
    """What a caller of the timed path holds after its last step: the camera pose and the surfel map (ef_get_pose, ef_map_download).
    A map above the budget is written as a fixed, seeded sample of its rows (in map order), with the full row count beside it."""
    os.makedirs(out_dir, exist_ok=True)
    T = np.asarray(ef.get_T_wc(), np.float64).reshape(4, 4)
    surfels = np.asarray(ef.downloadMap(), np.float32)
    n = len(surfels)
    cap = (DUMP_BYTES - 4096) // surfels[:1].nbytes if n else 0
    if n > cap:
        rows = np.sort(np.random.default_rng(0xEF0D).choice(n, cap, replace=False))
        surfels = surfels[rows]
    np.save(os.path.join(out_dir, "pose_T_wc.npy"), T)
    np.save(os.path.join(out_dir, "map_surfels.npy"), np.ascontiguousarray(surfels))
    np.save(os.path.join(out_dir, "map_count.npy"), np.array([n], np.float64))


def generate_frames(seed: int, n: int, w: int = W, h: int = H, ranks_on_host: int = 1):
    # the host cores are shared by all ranks of the node: 8 ranks x 16 workers would starve each other
    workers = max(1, min(16, (os.cpu_count() or 2) // max(1, ranks_on_host) - 1))
    with ProcessPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(_gen_frame, [(seed, k, w, h) for k in range(n)], chunksize=4))


def cpu_baseline(frames, budget_s: float = 20.0, w: int = W, h: int = H, poses_out=None):
    """Times the CPU oracle (the reference restated; the reference itself has no CPU path and cannot be built here)
    on the same frames, single thread, bounded to ~budget_s of CPU work.  Checker code used as a *baseline leg* only."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import efo
    def run(threads, budget, keep=None):
        efo.set_threads(threads)
        o = efo.Fusion(width=w, height=h, fx=528.0 * w / 640, fy=528.0 * w / 640, cx=320.0 * w / 640, cy=240.0 * w / 640)
        t0 = time.perf_counter()
        n = 0
        for rgb, depth, _ in frames:
            o.process_frame(rgb, depth, n)
            n += 1
            if keep is not None:
                keep.append(o.pose())     # (a 16-double copy per frame: nothing next to the ~0.5 s the frame took)
            if time.perf_counter() - t0 > budget and n >= 3:
                break
        return n, time.perf_counter() - t0

    def run_tracking_only(budget):
        """BASELINE.json configs[0]: one 640x480 pair, pose only — the tracker (initICP/initRGB pyramids excluded: SO(3) + 19
        ICP+RGB iterations, RGBDOdometry::getIncrementalTransformation) re-run on the state the second frame left behind."""
        efo.set_threads(1)
        o = efo.Fusion(width=w, height=h, fx=528.0 * w / 640, fy=528.0 * w / 640, cx=320.0 * w / 640, cy=240.0 * w / 640)
        for k in range(2):
            o.process_frame(frames[k][0], frames[k][1], k)
        od = o.odometry()
        T0 = frames[0][2]
        t0 = time.perf_counter()
        reps = 0
        while reps < 3 or time.perf_counter() - t0 < budget:
            od.track(T0)
            reps += 1
        od.h_ = None   # the handle belongs to the Fusion object
        return reps, time.perf_counter() - t0

    n, dt = run(1, budget_s * 0.6, poses_out)
    nt, dtt = run_tracking_only(budget_s * 0.15)
    cores = min(os.cpu_count() or 1, 32)   # threads are created per parallel loop; beyond ~32 the spawn cost eats the gain
    nm, dtm = run(cores, budget_s * 0.4) if cores > 1 else (n, dt)
    efo.set_threads(1)
    return {"value": n / dt, "unit": "frames/s", "cores": 1, "kind": "port",
            "sample": f"first {n} frames of the same {w}x{h} sequence through the oracle's full processFrame "
                      f"(tracking + fuse), single thread, {dt:.1f} s",
            "tracking_only": {"value": nt / dtt, "unit": "pairs/s", "cores": 1,
                              "sample": f"configs[0]: getIncrementalTransformation of one {w}x{h} pair (SO(3) + 10/5/4 ICP+RGB iterations, "
                                        f"pose only, no fuse) repeated {nt}x, single thread, {dtt:.1f} s"},
            "all_cores": {"value": nm / dtm, "cores": cores,
                          "sample": f"first {nm} frames, bilateral rows and the reduction blocks on {cores} std::threads "
                                    f"(the map passes stay serial), {dtm:.1f} s"}}


def _leave():
    """the line is out and everything is released: run the registered exit hooks, then skip the interpreter / GPU-runtime teardown"""
    import atexit
    sys.stdout.flush()
    sys.stderr.flush()
    if any("rocprof" in k.lower() or "rocprof" in v.lower() for k, v in os.environ.items()):
        return   # under rocprofv3 the tool writes its files from the runtime's own exit hooks: leave the normal way
    try:
        atexit._run_exitfuncs()
    except Exception:
        pass
    os._exit(0)


KT_FIELDS = None


def _kernel_time_struct():
    global KT_FIELDS
    if KT_FIELDS is None:
        class KT(C.Structure):
            _fields_ = [("name", C.c_char_p), ("avg_us", C.c_float), ("launches", C.c_int), ("bytes_per_launch", C.c_double),
                        ("bytes_per_launch_survey", C.c_double)]
        KT_FIELDS = KT
    return KT_FIELDS


def pmc_traffic_of(kernel_prefix, w, h):
    """HBM-side bytes per launch of a kernel from the COMMITTED PMC measurement (rocprofv3 PMC passes cannot run inside this process):
    profiles/pmc_traffic.json (640x480) / pmc_traffic_1280x960.json, written by tools/pmc_json.py from tools/pmc_traffic.sh's passes"""
    try:
        name = "pmc_traffic.json" if (w, h) == (W, H) else ("pmc_traffic_1280x960.json" if (w, h) == (1280, 960) else None)
        if name is None:
            return None, None
        with open(os.path.join(ROOT, "profiles", name)) as f:
            pj = json.load(f)
        # (k_track_ref is not k_track_ref_end; of a templated kernel's instances, the one that moves the most bytes: level 0's)
        hits = [rec for k, rec in pj.get("kernels", {}).items() if k == kernel_prefix or k.startswith(kernel_prefix + "<")]
        if hits:
            rec = max(hits, key=lambda r: r["traffic_bytes_per_launch"])
            what = f"; its launches: {rec['launches_are']}" if "launches_are" in rec else ""
            return int(rec["traffic_bytes_per_launch"]), (f"committed PMC measurement (profiles/{name}: {rec.get('source', pj.get('source', ''))}; FETCH_SIZE and WRITE_SIZE in separate "
                                                          f"rocprofv3 passes, calibrated on a known-byte kernel{what}), not measured in this run")
    except Exception:
        pass
    return None, None


def roofline_tracker(lib, ef, w=W, h=H):
    """the persistent tracker launch (k_track_ref / k_track_fast), the kernel that takes the most time of a frame: bytes, us, fraction of HBM peak"""
    KT = _kernel_time_struct()
    kt = KT()
    if not hasattr(lib, "ef_get_tracker_timing") or lib.ef_get_tracker_timing(ef.h, C.byref(kt)) != 0 or kt.launches <= 0:
        return None
    # `achieved` / `frac`: SURVEY 8(d)'s per-unit figure (48 B per pixel visit) x the visits of one launch; the kernel's own count (52 B: + the 4-byte packed
    # correspondence it writes and reads back) is the secondary key
    ach = kt.bytes_per_launch_survey / (kt.avg_us * 1e-6) / 1e9
    ach_own = kt.bytes_per_launch / (kt.avg_us * 1e-6) / 1e9
    name = kt.name.decode()
    traffic, tsrc = pmc_traffic_of(name.split(" ")[0], w, h)
    return {"bound": "hbm", "kernel": name, "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
            "avg_us": round(float(kt.avg_us), 2), "launches_sampled": int(kt.launches), "algorithmic_bytes_per_launch": int(kt.bytes_per_launch_survey),
            "algorithmic_bytes_per_launch_kernel_52B": int(kt.bytes_per_launch),
            "frac_kernel_52B": round(ach_own / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": tsrc,
            "timer": "dispatch begin/end timestamps (hipExtLaunchKernelGGL start/stop events) of the launch on the frames right behind the timed region (same replay, same map)",
            "note": "the dominant kernel of the timed region: a chain of 19 dependent Gauss-Newton iterations (two chip-wide exchanges and a 6x6 solve in double each) — "
                    "latency-bound, not bandwidth-bound; " + ("most of its algorithmic bytes are served by the L2s / MALL across iterations (traffic << algorithmic)"
                                                              if traffic is None or traffic < kt.bytes_per_launch else
                                                              "at this size the maps no longer stay in the L2s between iterations: the HBM-side traffic is the algorithmic bytes and a little more")}


def probe_frames_run(ef, lib, step, first, n, torch, w=W, h=H):
    """The replay goes on for n frames behind the timed region: a third of them timed one by one (events between frames, nothing sampled), a
    third with the persistent tracker launch sampled, a third with the launch-per-step script (bit-identical results, ef_set_persistent_tracker)
    so that the level-0 normal-equation kernel exists as a launch of its own and is sampled.  Returns per-frame times in ms."""
    third = max(1, n // 3)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(third + 1)]
    evs[0].record()
    for i, k in enumerate(range(first, first + third)):
        step(k)
        evs[i + 1].record()
    torch.cuda.synchronize()
    per_frame = [evs[i].elapsed_time(evs[i + 1]) for i in range(third)]
    lib.ef_kernel_timing(ef.h, C.c_int(1))
    for k in range(first + third, first + 2 * third):
        step(k)
    torch.cuda.synchronize()
    tracker = roofline_tracker(lib, ef, w, h)
    if tracker is not None:   # the persistent launch ran: sample the per-step script's kernels on the remaining frames
        ef.setPersistentTracker(False)
        lib.ef_kernel_timing(ef.h, C.c_int(1))
    for k in range(first + 2 * third, first + n):
        step(k)
    torch.cuda.synchronize()
    if tracker is not None:
        ef.setPersistentTracker(True)
    return per_frame, tracker


def rooflines(lib, ef, w, h, where):
    """(roofline of the level-0 normal-equation kernel, roofline of the IndexMap splat) from the engine's own dispatch-timestamp samples"""
    KT = _kernel_time_struct()
    roofline = roofline_splat = None
    kt = KT()
    if lib.ef_get_kernel_timing(ef.h, C.byref(kt)) == 0 and kt.launches > 0:
        # avg_us: the dispatches' own begin/end timestamps (hipExtLaunchKernelGGL start/stop events) of the sampled launches
        # -- the duration rocprofv3 --kernel-trace reports for the same kernel (profiles/)
        achieved = kt.bytes_per_launch / (kt.avg_us * 1e-6) / 1e9
        achieved_survey = kt.bytes_per_launch_survey / (kt.avg_us * 1e-6) / 1e9
        # HBM-side bytes per launch: rocprofv3 PMC passes cannot run inside this process, so this is the measurement
        # COMMITTED under profiles/ by tools/pmc_traffic.sh for this kernel and workload (see traffic_source), not a live value
        traffic, traffic_source = pmc_traffic_of(kt.name.decode().split(" ")[0], w, h)
        # (the sampled launch is the FIRST predictIndices of a frame, k_index_splat<false>; the second one, <true>, also carries the fusion's update pass)
        straffic, ssource = pmc_traffic_of("k_index_splat<false>", w, h)
        if straffic is None:
            straffic, ssource = pmc_traffic_of("k_index_splat", w, h)
        roofline = {"bound": "hbm", "kernel": kt.name.decode(), "achieved": round(achieved_survey, 1), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(achieved_survey / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
                    "avg_us": round(float(kt.avg_us), 3), "timer": "dispatch begin/end timestamps (hipExtLaunchKernelGGL start/stop events) of every level-0 launch of the " + where,
                    "launches_sampled": int(kt.launches), "algorithmic_bytes_per_launch": int(kt.bytes_per_launch_survey),
                    "algorithmic_bytes_per_launch_kernel_52B": int(kt.bytes_per_launch),
                    "frac_kernel_52B": round(achieved / HBM_PEAK_GBS, 4), "frac_of_achievable_6300": round(achieved_survey / 6300.0, 4)}
        ks = KT()
        if lib.ef_get_splat_timing(ef.h, C.byref(ks)) == 0 and ks.launches > 0:
            ach = ks.bytes_per_launch / (ks.avg_us * 1e-6) / 1e9
            roofline_splat = {"bound": "hbm", "kernel": ks.name.decode(), "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": straffic, "traffic_source": ssource, "avg_us": round(float(ks.avg_us), 3),
                              "launches_sampled": int(ks.launches), "algorithmic_bytes_per_launch": int(ks.bytes_per_launch)}
    return roofline, roofline_splat


class _StandInEngine:
    """--stand-in-engine: what bench.py calls on an engine, doing nothing but counting frames (tests/test_bench_multi_gloo.py: the
    multi-rank control flow of THIS file — barriers, the one collective, the exit of the ranks that do not print — on CPU with gloo)."""
    h = None

    def __init__(self, **kw):
        self.frames = 0

    def processFrameDevice(self, *a, **k):
        self.frames += 1
        time.sleep(0.002)

    processFrame = processFrameDevice

    def get_T_wc(self): return np.eye(4)
    def lastCount(self): return self.frames
    def downloadMap(self): return np.zeros((1, 12), np.float32)
    def getConfidenceThreshold(self): return 10.0
    def trajectory(self): return [np.eye(4)] * self.frames, None
    def close(self): pass
    def setPersistentTracker(self, on): pass
    def setTrackOnly(self, on): pass
    def setFusedStep(self, on): pass
    def setGraphReplay(self, on): pass
    def setInputOverlap(self, on): pass
    def setInputCuMask(self, n): pass


class _StandInLib:
    def __getattr__(self, name):
        return lambda *a, **k: -1     # every measurement hook: "nothing sampled"


class _StandInApi:
    LIB_PATH = "stand-in"
    ElasticFusion = _StandInEngine

    class DevBuf:
        class _P:
            value = 0
        p = _P()

        @staticmethod
        def from_array(a):
            return _StandInApi.DevBuf()

    @staticmethod
    def lib():
        return _StandInLib()

    @staticmethod
    def use_library(path):
        pass


class _NoGpu:
    """torch.cuda's part in this file, for --stand-in-engine"""
    @staticmethod
    def synchronize(): pass


def make_engine(api, w, h, device, stream, close_loops=False, graph=False, per_step=False, fused_step=False, input_overlap=0, round3=False):
    sc = w / 640.0
    ef = api.ElasticFusion(width=w, height=h, fx=528.0 * sc, fy=528.0 * sc, cx=320.0 * sc, cy=240.0 * sc, device=device, stream=stream,
                           maxSurfels=max(4 * 1024 * 1024, 6 * w * h), **(dict(closeLoops=True, timeDelta=200) if close_loops else {}))
    if per_step:
        ef.setPersistentTracker(False)
    if round3:
        ef.setPersistentTracker(2)
    if input_overlap:   # frame k + 1's input stage on a second stream (every input_overlap-th CU) beside frame k's fusion and prediction
        ef.setInputCuMask(input_overlap)
        ef.setInputOverlap(1)
    if fused_step:
        ef.setFusedStep(True)
    if graph:
        ef.setGraphReplay(True)
    if close_loops:   # the reference's closed-loop mode: fern database + global closure, then the local closure, built-in optimiser
        ef.useBuiltinLoopSolver(True)
        ef.enableGlobalClosure(seed=0)
    return ef


def sequences_on_one_gpu(api, frames, dev, w, h, device, m, steps, warmup, preroll):
    """m independent replays of the same frames sharing ONE GPU — m contexts, each with its own stream and its own host thread, running the
    launch-per-step tracker script (the persistent launch takes the whole chip: co-located sequences overlap better without it) — aggregate
    frames/s and whether all m ended on the same bits.  A side figure (BASELINE configs[3] puts one sequence on each GPU)."""
    import threading
    ctxs = []
    for _ in range(m):
        ef = make_engine(api, w, h, device, 0, per_step=True)   # stream 0 = the context creates its own non-blocking stream
        ctxs.append(ef)
    first = 1 + preroll + warmup
    go, done = threading.Barrier(m + 1), threading.Barrier(m + 1)
    errs = []

    def worker(ef):
        try:
            for k in range(first):
                ef.processFrameDevice(dev[k][0].p.value, dev[k][1].p.value, k * 33333)
            ef.synchronize()
            go.wait()
            for k in range(first, first + steps):
                ef.processFrameDevice(dev[k][0].p.value, dev[k][1].p.value, k * 33333)
            ef.synchronize()
        except Exception as e:   # a broken barrier would hang the others: report instead
            errs.append(repr(e))
            go.abort()
            done.abort()
            return
        done.wait()

    th = [threading.Thread(target=worker, args=(c,)) for c in ctxs]
    for t in th:
        t.start()
    go.wait()
    t0 = time.perf_counter()
    done.wait()
    dt = time.perf_counter() - t0
    for t in th:
        t.join()
    poses = [c.get_T_wc() for c in ctxs]
    counts = [c.lastCount() for c in ctxs]
    for c in ctxs:
        c.close()
    if errs:
        return {"error": errs[0]}
    return {"value": round(m * steps / dt, 2), "per_sequence": round(steps / dt, 2), "sequences": m, "steps": steps,
            "identical_results": bool(all(np.array_equal(poses[0], q) for q in poses) and len(set(counts)) == 1)}


def preseed(ef, seed, w, h, n, frame0):
    """a map of ~n surfels sampled on the scene's surfaces instead of the first frame's seeding"""
    from elasticfusion_amd import synth
    m = synth.sample_surfels(synth.Sequence(seed, width=w, height=h), n)
    ef.restore(dict(map=m, tick=2, qt=np.array([0, 0, 0, 1, 0, 0, 0], np.float64), rgb=frame0[0], depth=frame0[1]))
    return len(m)


def side_leg(torch, api, frames, dev, w, h, device, stream, steps, warmup, preroll, *, host_frames=False, close_loops=False, graph=False,
             track_only=False, per_step=False, seed=None, preseed_n=0, probe_frames=0):
    """one extra, separately timed replay of the same frames on a fresh engine (never the headline value) -> dict"""
    ef = make_engine(api, w, h, device, stream, close_loops=close_loops, graph=graph, per_step=per_step)
    k0 = 0
    if preseed_n:
        surfels = preseed(ef, seed, w, h, preseed_n, frames[0])
        k0 = 1

    def step(k):
        if host_frames:
            ef.processFrame(frames[k][0], frames[k][1], k * 33333)
        else:
            ef.processFrameDevice(dev[k][0].p.value, dev[k][1].p.value, k * 33333)

    first = k0 + (0 if preseed_n else 1) + preroll + warmup
    for k in range(k0, first):
        step(k)
    if track_only:
        ef.setTrackOnly(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(first, first + steps):
        step(k)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"value": round(steps / dt, 2), "ms_per_step": round(1e3 * dt / steps, 4), "steps": steps}
    if probe_frames:
        lib = api.lib()
        _, rt = probe_frames_run(ef, lib, step, first + steps, probe_frames, torch, w, h)
        r, rs = rooflines(lib, ef, w, h, f"last third of the {probe_frames} frames that follow the timed region (launch-per-step script)")
        out["roofline"], out["roofline_index_splat"], out["roofline_level0_per_step"] = rt, rs, r
    T = ef.get_T_wc()
    Tgt = frames[first + steps + probe_frames - 1][2]
    out["pose_err_vs_generating_traj_m"] = round(float(np.linalg.norm(T[:3, 3] - Tgt[:3, 3])), 5)
    out["surfels_end"] = int(ef.lastCount())
    if preseed_n:
        out["surfels_preseeded"] = int(surfels)
    ef.close()
    return out


def main():
    import faulthandler
    faulthandler.enable()
    # a wedged GPU runtime must not hold the caller for ever: 9 minutes for the GPU sections, then every thread's stack and out
    # (cancelled before the CPU baseline legs, which are bounded by their own budgets)
    faulthandler.dump_traceback_later(540, exit=True)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true", help="besides the headline: per-frame times and rooflines on the frames behind the timed region, "
                    "value_200_steps, the box calibration, the side legs of the N = 1 line and the CPU baseline (off by default)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="write what the timed path computed in its last step as DIR/<name>.npy "
                    "(pose_T_wc float64 4x4, map_surfels float32 [n, 12] or a seeded sample of its rows within 64 MB, map_count); rank 0")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU baseline")
    ap.add_argument("--probe-inside", action="store_true", help="development: sample the roofline kernels inside the timed region (1 frame in 8) "
                    "instead of on the frames that follow it")
    ap.add_argument("--frames-cache", default=None, help="development: keep the generated synthetic frames in this .npz between runs "
                    "(A/B runs of library variants on one GPU box); never needed for the headline")
    ap.add_argument("--width", type=int, default=W, help="1280 (with --height 960) = BASELINE.json configs[2]; NOT the headline metric")
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--host-frames", action="store_true", help="hand the frames over as HOST buffers (ef_process_frame: copy into pinned "
                    "staging + PCIe upload inside the timed region) - the PCIe-inclusive rate of DESIGN.md, never the headline value")
    ap.add_argument("--close-loops", action="store_true", help="closeLoops = true with the reference's default time window of 200 "
                    "frames: every frame also runs the global closure (fern match on the mid-frame view, keyframe store at the end) and the "
                    "local one (inactive-model prediction, second tracker, gates, built-in optimiser).  NOT the headline metric, which is "
                    "open loop (-o)")
    ap.add_argument("--graph", action="store_true", help="BASELINE.json configs[4]: the tracker's launches captured once into a hipGraph and "
                    "replayed (ef_set_graph_replay); bit-identical results, NOT the headline (measured: no faster, the host is not the limit)")
    ap.add_argument("--track-only", action="store_true", help="BASELINE.json configs[4]: odometry only on the map the pre-roll built "
                    "(ef_set_track_only during the timed region: pre-process, track, predict; no fusion) -> pairs/s")
    ap.add_argument("--library", default=None, help="'fast' = libefusion_hip_fast.so, the development variant (fused multiply-adds + fast summation order; retired from the shipped set in round 6), or a "
                    "path; default: the shipped libefusion_hip.so = the reference rounding (bit for bit the reference's own sources compiled "
                    "without contraction)")
    ap.add_argument("--preseed", type=int, default=0, help="SURVEY 8(d) config 3: start from a map of about this many surfels sampled on the "
                    "scene's surfaces (radius 4 mm, confidence 12) brought in with ef_map_upload + ef_restore_state instead of seeding from "
                    "the first frame; with --width 1280 --height 960 --preseed 1048576 = BASELINE.json configs[2], the HBM-bound map")
    ap.add_argument("--no-side-legs", action="store_true", help="with --full: skip the extra keys of the N = 1 line (host-frame path, reference-rounding "
                    "build, closed loop, odometry only, hipGraph replay, configs[4], configs[2])")
    ap.add_argument("--preroll", type=int, default=PREROLL, help="development (PMC passes on a pre-seeded map): untimed frames before the warm-up; "
                    "the driver's command never sets it (100: the map's steady state)")
    ap.add_argument("--input-overlap", type=int, default=0, help="development (A/B): the next frame's input stage on a second stream restricted to every "
                    "N-th CU (1 = unmasked), beside the previous frame's fusion (ef_set_input_overlap + ef_set_input_cu_mask)")
    ap.add_argument("--stand-in-engine", action="store_true", help="test hook (tests/test_bench_multi_gloo.py): no GPU, the gloo backend and an engine "
                    "that only counts frames - exercises this file's multi-rank control flow; the line says \"data\": \"stand-in\"")
    ap.add_argument("--fused-step", action="store_true", help="development (A/B): level-0 update step inside the correspondence-search launch "
                    "(ef_set_fused_step); results are bit-identical")
    ap.add_argument("--per-step-tracker", action="store_true", help="development (A/B): the tracker as one launch per step (68 launches) instead "
                    "of the persistent launch (ef_set_persistent_tracker(ctx, 0)); results are bit-identical")
    ap.add_argument("--round3-tracker", action="store_true", help="development (A/B, reference-order builds): round 3's tracker script — the small levels + SO(3) "
                    "as one launch of 128 workgroups (k_track_small), three launches per level-0 iteration (ef_set_persistent_tracker(ctx, 2)); bit-identical")
    a = ap.parse_args()
    w, h = a.width, a.height

    from elasticfusion_amd import multi
    rank, local_rank, world = multi.rank_info()
    if world != a.gpus and world > 1:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if world > 1:   # N ranks enqueue ~20 k launches/s each from one host: every rank keeps to its own share of the cores
        multi.pin_rank_to_cores(local_rank, world)
    plain = not (a.stand_in_engine or a.host_frames or a.close_loops or a.graph or a.track_only or a.library or a.preseed or a.per_step_tracker or a.round3_tracker or a.probe_inside or a.fused_step or a.input_overlap or a.preroll != PREROLL)
    side = a.full and world == 1 and plain and (w, h) == (W, H) and not a.no_side_legs   # the extra keys ride on the default N = 1 line only
    # the frames behind the timed region: sampled kernels (--full), or nothing but the headline
    probe = PROBE_FRAMES if a.full and not a.probe_inside else 0

    # synthetic frames first: the generator forks worker processes, which must happen before HIP / RCCL are initialised
    # frame 0 seeds the map (tick 1); pre-roll and warm-up are never timed; with --full the last PROBE_FRAMES frames continue the same replay
    # with the per-kernel sampling switched on (a sampled launch carries profiling timestamps, which the timed region is kept free of)
    self_check = SELF_CHECK if a.full and world == 1 and plain and (w, h) == (W, H) and a.steps < SELF_CHECK else 0
    n_frames = 1 + a.preroll + a.warmup + a.steps + probe + self_check
    seed = multi.sequence_seed(rank)
    frames = replay_frames(seed, n_frames, w, h, ranks_on_host=world, cache=f"{a.frames_cache}.{rank}" if a.frames_cache else None)
    big = None
    BIG = dict(w=1280, h=960, preroll=16, warmup=24, steps=60, probe=8, preseed=1 << 20)   # (a long warm-up: the GPU idles for seconds while the host samples the map)
    if side:   # configs[2] for the extra key: 1280x960, ~1 M pre-seeded surfels (fewer frames: the map is mature from the start)
        nb = 1 + BIG["preroll"] + BIG["warmup"] + BIG["steps"] + BIG["probe"]
        big = replay_frames(seed, nb, BIG["w"], BIG["h"], cache=f"{a.frames_cache}.{rank}" if a.frames_cache else None)

    import torch
    import torch.distributed as dist
    if a.stand_in_engine:
        if world > 1:
            multi.init_process_group("gloo", local_rank)
        api, build, gpu, stream, stats_device = _StandInApi, None, _NoGpu, 0, None
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU: the HIP engine has no CPU fallback")
        torch.cuda.set_device(local_rank)
        if world > 1:
            multi.init_process_group("nccl", local_rank)

        from elasticfusion_amd import api, build
        if a.library:
            if a.library == "fast" and not os.path.exists(build.FAST_LIB):
                build.build_variant("fast", [])   # (a development variant since round 6: not part of build())
            api.use_library(build.FAST_LIB if a.library == "fast" else a.library)

        # a real (non-null) stream, made torch's current one: the engine enqueues on it, torch.cuda.synchronize() covers it,
        # and it can be captured into a hipGraph (--graph), which the legacy null stream cannot
        tstream = torch.cuda.Stream()
        torch.cuda.set_stream(tstream)
        stream = tstream.cuda_stream
        gpu, stats_device = torch.cuda, "cuda"
    ef = make_engine(api, w, h, local_rank, stream, close_loops=a.close_loops, graph=a.graph, per_step=a.per_step_tracker, fused_step=a.fused_step,
                     input_overlap=a.input_overlap, round3=a.round3_tracker)
    dev = upload_frames(api, frames)
    k0 = 0
    n_pre = 0
    if a.preseed:
        n_pre = preseed(ef, seed, w, h, a.preseed, frames[0])
        k0 = 1

    def step(k):
        if a.host_frames:
            ef.processFrame(frames[k][0], frames[k][1], k * 33333)
        else:
            ef.processFrameDevice(dev[k][0].p.value, dev[k][1].p.value, k * 33333)

    first_timed = 1 + a.preroll + a.warmup
    for k in range(k0, first_timed):
        step(k)
    if a.track_only:
        ef.setTrackOnly(True)
    # per-kernel HIP-event sampling of the dominant kernel inside the timed region (1 frame in 8)
    lib = api.lib()
    if a.probe_inside:
        lib.ef_kernel_timing(ef.h, C.c_int(8))
    gpu.synchronize()
    if world > 1:
        dist.barrier()
    gpu.synchronize()
    t0 = time.perf_counter()
    for k in range(first_timed, first_timed + a.steps):
        step(k)
    gpu.synchronize()
    if world > 1:
        dist.barrier()
    gpu.synchronize()
    dt = time.perf_counter() - t0
    if a.dump_outputs and rank == 0:   # the state the last timed step left behind, before anything else runs on this engine
        dump_outputs(ef, a.dump_outputs)
    per_frame_ms, rtracker = [], None
    if probe and a.stand_in_engine:
        for k in range(first_timed + a.steps, first_timed + a.steps + probe):
            step(k)
    elif probe:   # the same replay goes on: per-frame times, then the sampled kernels (see probe_frames_run)
        per_frame_ms, rtracker = probe_frames_run(ef, lib, step, first_timed + a.steps, probe, torch, w, h)

    # pose error of the timed run against the generating trajectory (sanity, not the parity bar)
    T = ef.get_T_wc()
    Tgt = frames[first_timed + a.steps - 1 + probe][2]
    err_t = float(np.linalg.norm(T[:3, 3] - Tgt[:3, 3]))
    count = ef.lastCount()
    stable = int((ef.downloadMap()[:, 3] > ef.getConfidenceThreshold()).sum()) if rank == 0 and a.full else None
    roofline = roofline_splat = None
    if a.full or a.probe_inside:
        roofline, roofline_splat = rooflines(lib, ef, w, h, (f"last third of the {PROBE_FRAMES} frames that follow the timed region (same replay, same map; "
                                                              "launch-per-step script, bit-identical results)"
                                                             if not a.probe_inside else "sampled frames inside the timed region"))
    value_200 = None
    if self_check and not a.stand_in_engine and not a.probe_inside:   # the same replay goes on: one more, longer timed region (never `value`)
        lib.ef_kernel_timing(ef.h, C.c_int(0))
        k1 = first_timed + a.steps + PROBE_FRAMES
        gpu.synchronize()
        t1 = time.perf_counter()
        for k in range(k1, k1 + self_check):
            step(k)
        gpu.synchronize()
        value_200 = self_check / (time.perf_counter() - t1)

    # the only collective: 40 B per rank over xGMI (RCCL all_gather): seconds, frames, pose error, surfels, the sequence's seed
    allstats = multi.gather_stats([dt, float(a.steps), err_t, float(count), float(seed)], device=stats_device)
    if rank != 0:
        ef.close()
        if world > 1:
            dist.destroy_process_group()
        _leave()
        return
    agg = multi.aggregate(allstats)
    t_max, value = agg["t_max"], agg["value"]
    calib = None
    if a.full:
        try:   # box calibration (GPU boxes of the pool differ by 10-20 %): what an empty kernel and a 16 MiB copy cost on THIS box, back to back
            if a.stand_in_engine:
                raise RuntimeError("stand-in engine: nothing to calibrate")
            e_us, s_us = C.c_float(0), C.c_float(0)
            if lib.ef_dev_calibrate(C.c_void_p(stream), C.byref(e_us), C.byref(s_us)) == 0:
                calib = {"empty_kernel_us": round(e_us.value, 3), "copy_16MiB_us": round(s_us.value, 3),
                         "copy_16MiB_GBps": round(2 * 16.777216e6 / (s_us.value * 1e-6) / 1e9, 1) if s_us.value > 0 else None,
                         "what": "200 back-to-back launches each on the bench's stream, averaged between two events (launch gaps included)"}
        except Exception as e:
            calib = {"error": repr(e)}
    mode = ("HOST frames (pinned staging + PCIe upload timed), " if a.host_frames else "") + \
           ("closeLoops (fern database + global closure + local closure every frame, timeDelta 200), " if a.close_loops else "open loop, ") + \
           ("tracker replayed from a hipGraph, " if a.graph else "") + ("ODOMETRY ONLY in the timed region (no fusion), " if a.track_only else "") + \
           ("one launch per tracker step (round-2 script), " if a.per_step_tracker else "") + ("round 3's tracker script (k_track_small + launch-per-step level 0), " if a.round3_tracker else "") + ("level-0 update step fused into the search launch, " if a.fused_step else "") + \
           (f"library {os.path.basename(api.LIB_PATH)}, " if a.library else "reference-rounding build (libefusion_hip.so: no fused multiply-add, the reference's summation order), ") + \
           (f"map pre-seeded with {n_pre} surfels sampled on the scene (radius 4 mm, confidence 12), " if a.preseed else "")
    out = {
        "metric": f"frames/s per GPU, {w}x{h} 3-level ICP+fuse",
        "value": round(value, 2),
        "unit": "frames/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(1e3 * t_max / a.steps, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "stand-in" if a.stand_in_engine else "synthetic",
        "parity": ("bit-exact against the reference's SOURCE semantics: the timed library is the reference rounding (every result equal to the reference's own "
                   "sources compiled by g++ with -ffp-contract=off; tests/test_gpu_vs_reference.py).  Caveat: a real nvcc / GLSL build fuses multiply-adds where its "
                   "compiler chooses, which cannot be observed here; a different FMA placement from identical state lands outside 1e-4 m / 1e-4 rad on 15 of 113 "
                   "one-frame checkpoints (profiles/r05_parity_factorial.json) — against a CUDA-built binary expect 'inside the bar on ~87 % of frames, "
                   "indistinguishable in accuracy', not bit equality" if not a.library else "see --library"),
        "config": {"workload": f"{w}x{h} synthetic RGB-D replay (box+spheres, Lissajous trajectory), " + mode +
                               "SO(3)+ICP+RGB 3-level tracking (10/5/4 its) + surfel fuse/clean/predict; "
                               + ("stand-in for configs[1] (dyson_lab.klg is not available offline)" if (w, h) == (W, H) else
                                  "configs[2]: 1280x960 stream"),
                   "resolution": [w, h], "sequences": world, "rccl_world_size": (dist.get_world_size() if world > 1 else 1),
                   "preroll_frames": a.preroll, "surfels_end": int(count),
                   "pose_err_vs_generating_traj_m": round(err_t, 5),
                   "per_rank_fps": [round(x, 2) for x in agg["per_rank_fps"]],
                   "sequence_seeds": [hex(int(x)) for x in allstats[:, 4]]},
        # the dominant kernel of the timed region (the persistent tracker launch); when the launch-per-step script was timed (--per-step-tracker,
        # --graph, rgbOnly) there is no such launch and the level-0 normal-equation kernel stands here
        "roofline": rtracker if rtracker is not None else roofline,
        "roofline_index_splat": roofline_splat,
        "roofline_level0_per_step": roofline if rtracker is not None else None,
        "value_200_steps": (round(value_200, 2) if value_200 else None),
        "box_calibration": calib,
        "frame_time_ms": ({"min": round(min(per_frame_ms), 4), "median": round(float(np.median(per_frame_ms)), 4), "max": round(max(per_frame_ms), 4),
                           "frames": len(per_frame_ms), "what": "GPU time of single frames (events between frames) right behind the timed region"}
                          if per_frame_ms else None),
    }
    out["config"]["stable_surfels_end"] = stable
    gpu_poses = None
    try:
        if a.full:   # (for the ATE against the CPU baseline)
            gpu_poses, _ = ef.trajectory()
    except Exception:
        pass
    ef.close()
    if side:
        # Extra keys of the N = 1 line: the same frames replayed on fresh engines in the other modes a reader of the headline asks
        # about.  Each leg is timed on its own after the headline's clock has stopped; none of them is `value`.
        legs = {}
        common = dict(steps=a.steps, warmup=a.warmup, preroll=a.preroll)
        try:
            legs["host_frames_fps"] = side_leg(torch, api, frames, dev, w, h, local_rank, stream, host_frames=True, **common)
            legs["host_frames_fps"]["what"] = "the B1 signature: frames handed over as HOST pointers (ef_process_frame: pinned staging + PCIe upload inside the timed region)"
            out["host_frames_fps"] = legs["host_frames_fps"]["value"]   # (top level too: the drop-in signature's rate, PCIe inclusive; never `value`)
            legs["graph_replay_fps"] = side_leg(torch, api, frames, dev, w, h, local_rank, stream, graph=True, **common)
            legs["graph_replay_fps"]["what"] = "BASELINE configs[4]: the tracker's launches replayed from a hipGraph (ef_set_graph_replay), full frame"
            legs["track_only_pairs_per_s"] = side_leg(torch, api, frames, dev, w, h, local_rank, stream, track_only=True, **common)
            legs["track_only_pairs_per_s"]["what"] = ("BASELINE configs[4] / configs[0] on the GPU: odometry only (pre-process + SO(3) + 19 ICP+RGB iterations + "
                                                      "prediction at the new pose) on the mature map, no fusion; beside cpu_baseline.tracking_only")
            legs["config4_graph_track_only_pairs_per_s"] = side_leg(torch, api, frames, dev, w, h, local_rank, stream, graph=True, track_only=True, **common)
            legs["config4_graph_track_only_pairs_per_s"]["what"] = ("BASELINE configs[4] AS WRITTEN: open-loop odometry only (ef_set_track_only: pre-process + SO(3) + 19 ICP+RGB "
                                                                    "iterations + prediction, no fusion) WITH the tracker's launches replayed from a hipGraph (ef_set_graph_replay)")
            legs["per_step_tracker_fps"] = side_leg(torch, api, frames, dev, w, h, local_rank, stream, per_step=True, **common)
            legs["per_step_tracker_fps"]["what"] = "the launch-per-step tracker script (68 launches instead of one persistent launch) on this box, for the persistent launch's A/B"
            legs["close_loops_fps"] = side_leg(torch, api, frames, dev, w, h, local_rank, stream, close_loops=True, **common)
            legs["close_loops_fps"]["what"] = "the reference's DEFAULT mode (closeLoops = true, timeDelta 200): fern database + global closure + local closure every frame"
        except Exception as e:   # never let a side figure cost the line
            legs["error"] = repr(e)
        try:
            legs["four_sequences_on_one_gpu_fps"] = sequences_on_one_gpu(api, frames, dev, w, h, local_rank, 4, a.steps, a.warmup, a.preroll)
            legs["four_sequences_on_one_gpu_fps"]["what"] = ("AGGREGATE frames/s of four independent replays sharing this GPU (four contexts, four host threads, launch-per-step "
                                                             "tracker scripts; results identical across the four): what a server with more streams than GPUs gets per device.  With --steps 20 the "
                                                             "timed region is ~25 ms and thread start-up skew understates it: 150-step runs read 1732 / 2525 / 3715 for 1 / 2 / 4 replays (profiles/r05l_shared_gpu.jsonl)")
        except Exception as e:
            legs["four_sequences_on_one_gpu_fps"] = {"error": repr(e)}
        try:
            bdev = upload_frames(api, big)
            leg = side_leg(torch, api, big, bdev, BIG["w"], BIG["h"], local_rank, stream, BIG["steps"], BIG["warmup"], BIG["preroll"],
                           seed=seed, preseed_n=BIG["preseed"], probe_frames=BIG["probe"])
            leg["what"] = ("BASELINE configs[2] as SURVEY 8(d) defines it: 1280x960 stream on a map pre-seeded with ~1 M surfels (ef_map_upload of "
                           "surfels sampled on the scene, radius 4 mm, confidence 12); rooflines by the engine's dispatch-timestamp events")
            legs["config2_1280x960_1M"] = leg
            del bdev
        except Exception as e:
            legs["config2_1280x960_1M"] = {"error": repr(e)}
        out["side_legs"] = legs
    faulthandler.cancel_dump_traceback_later()
    if a.full and not a.no_cpu_baseline and world == 1:   # rank 0 at N=1 only (the scaling runs reuse the N=1 figure)
        oracle_poses = []
        out["cpu_baseline"] = cpu_baseline(frames[: min(len(frames), 40)], w=w, h=h, poses_out=oracle_poses)
        # BASELINE.json's metric names "ATE vs reference pose": the CPU leg above ran the reference's restatement over the first frames
        # of this very replay, so the GPU run's logged trajectory can be held against it frame by frame (bit-identical expected: 0.0)
        try:
            m = min(len(oracle_poses), len(gpu_poses)) if gpu_poses is not None else 0
            if m > 0 and not a.close_loops and not a.preseed and not a.library:
                d = np.array([gpu_poses[k][:3, 3] - oracle_poses[k][:3, 3] for k in range(m)])
                rot = max(float(np.abs(gpu_poses[k][:3, :3] - oracle_poses[k][:3, :3]).max()) for k in range(m))
                out["ate_vs_oracle"] = {"rmse_m": float(np.sqrt((d * d).sum(1).mean())), "max_m": float(np.abs(d).max()), "max_rotation_entry_diff": rot,
                                        "frames": m, "what": "logged GPU poses of the first frames of this run against the CPU oracle's poses on the same frames"}
        except Exception as e:   # never let the side figure cost the line
            out["ate_vs_oracle"] = {"error": repr(e)}
    print(json.dumps(out), flush=True)
    del dev
    gpu.synchronize()
    if world > 1:
        dist.destroy_process_group()
    _leave()


if __name__ == "__main__":
    main()
