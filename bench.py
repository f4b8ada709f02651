#!/usr/bin/env python
"""bench.py - rollout steps/s of the ACE2-shape 1-degree SFNO on N MI355X (one ensemble member per GPU).

    python bench.py --gpus 1 --steps 40 --warmup 5
    python bench.py --gpus 1 --steps 40 --warmup 5 --dump-outputs DIR     # + the last timed step's outputs as DIR/<name>.npy
    python bench.py --gpus 1 --steps 40 --warmup 5 --full                  # + everything beyond the headline figure
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one pass of the whole hot path over one synthetic state: gather+normalise the 44 input fields,
the SFNO forward (8 blocks, embed 384, 180x360, fp32), scatter+denormalise the 50 output fields, feed the 36
prognostic fields back.  Inputs are resident in HBM before the timed region.  Prints ONE JSON line on rank 0.

A plain run does only what the headline figure needs: set up, warm up, time the K steps of the headline precision, dump the
outputs if asked, print the line (`roofline`, `roofline_sht`, `stages` and `cpu_baseline` are null in it).  `--full` adds the
rest: the second precision mode, per-stage HIP-event times and the rooflines, the CPU baseline and the extra legs (one-year rollout,
S80 state).
"""

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

# ---- workload: BASELINE.json configs[1] ("ACE2-ERA5-shape 1-degree SFNO ... one MI355X, hipGraph-captured step")
ACE2 = dict(embed_dim=384, num_layers=8, operator_type="dhconv", scale_factor=1, data_grid="legendre-gauss")
IMG = (180, 360)
N_FORCING, N_PROGNOSTIC, N_DIAGNOSTIC = 8, 36, 14       # 44 in / 50 out, 58 distinct names
PEAK_MFMA_F32 = 157.3      # TFLOP/s dense, v_mfma_f32_32x32x2_f32 (MI355X_MICROARCH.md)
PEAK_HBM = 8000.0          # GB/s spec (6290 achievable)


def names():
    forcing = [f"forcing_{i}" for i in range(N_FORCING)]
    prog = [f"prog_{i}" for i in range(N_PROGNOSTIC)]
    diag = [f"diag_{i}" for i in range(N_DIAGNOSTIC)]
    return forcing, prog, diag


def stage_model(C=384, H=180, W=360, L=180, M=181, hid=768, cin=44, cout=50):
    """(flops, algorithmic bytes, moved bytes) per launch of each stage (DESIGN.md section 'Kernels'), B = 1."""
    act = C * H * W * 4
    tiles = (H * W + 31) // 32                      # fc2 emits one statistics partial (16 B) per 32-pixel tile and channel
    groups = 8 * (32 // (C // 128) + (32 - (32 // (C // 128)) * (C // 128))) if C % 128 == 0 else tiles   # inner skip: one per pixel group
    coef = C * L * M * 8
    tab = M * L * H * 4
    fft_flops = 2 * 21_000 * C * H      # two-level 20 x 18 FFT on the vector ALUs: ~21 k fp32 FMAs per row (csrc/fft.hip)
    tri = C * 8 * sum(min(l + 1, M) for l in range(L))   # coefficients with l >= m only: what D / E hold (csrc/strip_fold.hip)
    tabf = 8_600_000 if (H, L, M) == (180, 180, 181) else tab // 2 + tab // 8   # packed folded table (strip_pack.h): 8.6 MB at 1 degree
    wf = 2 * C * C * L * 4
    f = {
        # name: (flops, algorithmic HBM bytes = SURVEY 8(d): every operand once, dense, moved bytes = what the layout of this
        # build transfers: triangular D / E, folded packed table)
        "forward_transform.dft": (fft_flops, act + coef, act + coef),
        "forward_transform.legendre": (2 * 2 * C * M * L * H, 2 * coef + tab, coef + tabf + tri),
        "dhconv": (8 * C * C * L * M, 2 * coef + wf, 2 * tri + wf),      # coef_in + Wf (212 MB) + coef_out
        "inverse_transform.legendre": (2 * 2 * C * M * L * H, 2 * coef + tab, coef + tabf + tri),
        "inverse_transform.dft": (fft_flops, act + coef, act + coef),
        "inner_skip+activation": (2 * C * C * H * W, 3 * act),
        "mlp.fc1": (2 * hid * C * H * W, act + hid * H * W * 4),
        "mlp.fc2+outer_skip": (2 * hid * C * H * W, 2 * act + hid * H * W * 4),
        # f16x3 mode: the instance norms are a finaliser over the statistics partials of the producing convolution (+ the
        # re-packing of the norm-folded fc1 weight for norm1); no pass over an activation (fp32 mode: one pass, 99.5 MB)
        "norm0_stats": (8 * tiles * C, tiles * C * 16 + 4 * C * 4),
        "norm1_stats": (8 * groups * C + 2 * hid * C, groups * C * 16 + 2 * hid * C * 4 + 4 * C * 4),
        # (moved: input + hidden planes written and read + h0 as planes; the fp32 copy of h0 is no longer written - conv_ws mode 8)
        "encoder": (2 * (cin * C + C * C) * H * W, cin * H * W * 4 + 4 * act, cin * H * W * 4 + 3 * act),
        "decoder": (2 * ((C + cin) * C + C * cout) * H * W, 3 * act + (cin + cout) * H * W * 4),
    }
    return {k: (v if len(v) == 3 else (v[0], v[1], v[1])) for k, v in f.items()}


def hook_names():
    """ACE2-style variable names (8 model levels) with the same 44 / 50 channel counts, so that the post-step physics of a
    real checkpoint (atmosphere corrector + prescribed-SST ocean) finds its fields: --hooks."""
    lv = range(8)
    forcing = ["DSWRFtoa", "HGTsfc", "ocean_fraction", "land_fraction", "sea_ice_fraction", "forcing_5", "forcing_6", "forcing_7"]
    prog = (["PRESsfc", "surface_temperature"] + [f"specific_total_water_{k}" for k in lv] + [f"air_temperature_{k}" for k in lv]
            + [f"eastward_wind_{k}" for k in lv] + [f"northward_wind_{k}" for k in lv] + ["TMP2m", "Q2m"])
    diag = ["PRATEsfc", "LHTFLsfc", "SHTFLsfc", "tendency_of_total_water_path_due_to_advection", "DSWRFsfc", "USWRFsfc",
            "DLWRFsfc", "ULWRFsfc", "ULWRFtoa", "USWRFtoa", "diag_10", "diag_11", "diag_12", "diag_13"]
    assert (len(forcing), len(prog), len(diag)) == (N_FORCING, N_PROGNOSTIC, N_DIAGNOSTIC)
    return forcing, prog, diag


def build_stepper(dev, seed, hooks=False):
    import ace_amd
    from ace_amd.step import NormalizationConfig

    if hooks:
        import numpy as np
        forcing, prog, diag = hook_names()
        in_names, out_names = forcing + prog, prog + diag
        # normalisation that keeps the synthetic state in a physically meaningful range (pressure ~1e5 Pa, water ~1e-3 ...)
        means = {k: 0.1 for k in in_names + out_names}
        stds = {k: 1.1 for k in in_names + out_names}
        means.update({"PRESsfc": 1.0e5, "surface_temperature": 288.0, "HGTsfc": 300.0, "DSWRFtoa": 340.0})
        stds.update({"PRESsfc": 1.0e3, "surface_temperature": 10.0, "HGTsfc": 100.0, "DSWRFtoa": 100.0})
        for k in range(8):
            means[f"specific_total_water_{k}"], stds[f"specific_total_water_{k}"] = 3.0e-3, 1.0e-4
            means[f"air_temperature_{k}"], stds[f"air_temperature_{k}"] = 250.0, 5.0
        cfg = ace_amd.SingleModuleStepConfig(
            builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet", config=ACE2),
            in_names=in_names, out_names=out_names, normalization=NormalizationConfig(means=means, stds=stds),
            ocean={"surface_temperature_name": "surface_temperature", "ocean_fraction_name": "ocean_fraction"},
            corrector={"conserve_dry_air": True, "moisture_budget_correction": "advection_and_precipitation",
                       "force_positive_names": ["PRATEsfc"] + [f"specific_total_water_{k}" for k in range(8)],
                       "total_energy_budget_correction": {"method": "constant_temperature", "constant_unaccounted_heating": 0.0}})
        lat, _ = np.polynomial.legendre.leggauss(IMG[0])
        lat = torch.tensor(np.degrees(np.arcsin(lat)), dtype=torch.float32)
        ak = torch.linspace(0.0, 2.0e4, 9).flip(0) * torch.linspace(0.0, 1.0, 9)      # 9 interfaces, ak(surface) = 0
        bk = torch.linspace(0.0, 1.0, 9)
        info = ace_amd.DatasetInfo(IMG, lat=lat, lon=torch.arange(IMG[1]) * (360.0 / IMG[1]), ak=ak, bk=bk)
        torch.manual_seed(seed)
        stepper = ace_amd.Stepper.from_config(cfg, info, device=dev)
        stepper.set_eval()
        return stepper, forcing, prog, diag
    forcing, prog, diag = names()
    in_names = forcing + prog
    out_names = prog + diag
    allnames = forcing + prog + diag
    cfg = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet", config=ACE2),
        in_names=in_names, out_names=out_names,
        normalization=NormalizationConfig(means={k: 0.1 for k in allnames}, stds={k: 1.1 for k in allnames}),
    )
    torch.manual_seed(seed)  # weights generated on CPU exactly as the reference initialises them, then uploaded
    stepper = ace_amd.Stepper.from_config(cfg, ace_amd.DatasetInfo(IMG), device=dev)
    stepper.set_eval()
    return stepper, forcing, prog, diag


def cpu_baseline(stepper, x_cpu, budget_s=45.0):
    """The reference CPU path, restated (oracle 'port': the same torch-CPU op sequence as fme's SFNO forward, pinned on the
    reference's goldens), timed on this box's host cores in the same run (SURVEY 8(d) / BASELINE.md protocol: 1 warm-up + 3 timed
    steps).  It is a stated baseline and should be the fastest this host can do: after one untimed warm-up one WHOLE forward step is
    timed at 32 and at 64 threads (a matrix-multiply probe does not predict the forward's best thread count - round 2 picked 64 and
    got 13 s where 32 threads take 7 s; 128 threads were never faster), then two more at the faster count: three timed steps there,
    reported as best / median / worst.  Bounded: no forward starts once `budget_s` seconds of CPU work would be exceeded."""
    from oracle.sfno import SFNOConfig, SFNOOracle

    ncpu = os.cpu_count() or 1
    cands = [t for t in (32, 64) if t <= ncpu] or [ncpu]
    cfg = SFNOConfig(in_chans=N_FORCING + N_PROGNOSTIC, out_chans=N_PROGNOSTIC + N_DIAGNOSTIC, img_shape=IMG,
                     embed_dim=384, num_layers=8, operator_type="dhconv")
    state = {k: v.detach().cpu() for k, v in stepper.modules[0].state_dict().items()}
    net = SFNOOracle(cfg, state)
    times = {}                                                    # threads -> timed steps
    with torch.no_grad():
        torch.set_num_threads(cands[0])
        t0 = time.perf_counter()
        y = net(x_cpu)                                            # warm-up (first-touch allocations, table construction)
        warm = time.perf_counter() - t0
        spent = warm

        def timed(th):
            nonlocal spent, y
            expect = min(times.get(th, [warm]))
            if spent + expect > budget_s:
                return False
            torch.set_num_threads(th)
            t0 = time.perf_counter()
            y = net(x_cpu)
            dt = time.perf_counter() - t0
            spent += dt
            times.setdefault(th, []).append(dt)
            return True

        for th in cands:
            timed(th)
        if times:
            best_th = min(times, key=lambda t: min(times[t]))
            while len(times[best_th]) < 3 and timed(best_th):
                pass
    if not times:
        times[cands[0]] = [warm]
    threads = min(times, key=lambda t: min(times[t]))
    at_best = sorted(times[threads])
    best = at_best[0]
    return dict(value=1.0 / best, unit="steps/s", cores=threads, host_logical_cores=ncpu, kind="port",
                seconds_per_step_by_threads={str(k): round(min(v), 3) for k, v in sorted(times.items())},
                seconds_per_step={"best": round(best, 3), "median": round(at_best[len(at_best) // 2], 3), "worst": round(at_best[-1], 3),
                                  "timed_steps_at_best": len(at_best), "warmup": round(warm, 3), "cpu_seconds_spent": round(spent, 1)},
                sample=f"whole forward steps of the same ACE2-shape network (B=1, fp32, torch-CPU ops): 1 warm-up, one timed step at "
                       f"each of {sorted(times)} threads, {len(at_best)} timed steps at the faster count, within a {budget_s:.0f} s budget; "
                       f"{best:.2f} / {at_best[len(at_best) // 2]:.2f} / {at_best[-1]:.2f} s/step (best / median / worst) on {threads} of "
                       f"{ncpu} host threads"), y


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def timed_window(eng, ens, dist, dev, K, Wm, world):
    """The rank orchestration of one measurement, identical on every rank: untimed warm-up (graph capture; for N > 1 two
    all-reduces - RCCL sets its channels / buffers up on the first collective of a size, the second gives its steady-state
    device time), then [sync; barrier; sync; K steps; for N > 1 ONE ensemble-mean all-reduce of the final state on the side
    stream (reference cadence: fme/ace/aggregator/one_step/ensemble.py:93-112,299); sync; barrier; sync], then the MAX of the
    wall time over ranks (fme/core/distributed/torch_distributed.py:130-132 reductions).  `eng` needs: graph_mode,
    run_window(), _enqueue_step(s, use_library_graph), out (name -> (B, T, H, W)), out_names - ace_amd.rollout.RolloutEngine,
    or the stub engine of tests/test_bench_ranks_cpu.py that drives this very function under gloo with world_size 2.
    Returns (seconds, steady-state all-reduce ms or None)."""
    T = K

    def window(n_steps):
        for s in range(n_steps):
            eng._enqueue_step(s % T, eng.graph_mode == "step")

    allreduce_ms = None
    with torch.no_grad():
        if eng.graph_mode == "window":
            eng.run_window()                                      # untimed: captures the K-step window and replays it
        else:
            window(max(Wm, 1))                                    # untimed warm-up (graph capture happens here)
        if world > 1:
            ens.submit([eng.out[n][0, 0] for n in eng.out_names])
            ens.result()
            ens.submit([eng.out[n][0, 0] for n in eng.out_names])
            allreduce_ms = ens.last_allreduce_ms()
        _sync(dev)
        dist.barrier()
        _sync(dev)
        t0 = time.perf_counter()
        if eng.graph_mode == "window":
            eng.run_window()
        else:
            window(K)
        if world > 1:
            ens.submit([eng.out[n][0, K - 1] for n in eng.out_names])
            ens.result()
        _sync(dev)
        dist.barrier()
        _sync(dev)
        dt = time.perf_counter() - t0
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    dist.reduce_max(tmax)
    return float(tmax.item()), allreduce_ms


def gather_rank_records(dist, dev, rank, local_rank, world, allreduce_ms):
    """who ran what: one record per rank (device, backend, its all-reduce time), gathered on every rank"""
    dev = torch.device(dev)
    mine = {"rank": rank, "local_rank": local_rank,
            "device": torch.cuda.get_device_name(dev) if dev.type == "cuda" else "cpu",
            "backend": (torch.distributed.get_backend() if dist.is_distributed() else "none"),
            "allreduce_ms": allreduce_ms}
    if not dist.is_distributed():
        return [mine]
    ranks_info = [None] * world
    torch.distributed.all_gather_object(ranks_info, mine)
    return ranks_info


def multi_gpu_block(world, ranks_info, allreduce_bytes):
    return {"world_size": world, "ranks": ranks_info, "allreduce_bytes": allreduce_bytes,
            "allreduce_stream": "side stream, event-ordered after the step stream (ace_amd/distributed.py AsyncEnsembleMean)",
            "timing": "max over ranks of [barrier; K steps; one ensemble-mean all-reduce; sync; barrier]"}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(eng, K, out_dir):
    """--dump-outputs: every output plane the timed path wrote in its last timed step (window position K - 1), as the caller of
    the engine receives it in `eng.out`, one float32 `<name>.npy` per field.  The ACE2-shape state is 50 x 180 x 360 x 4 B = 13 MB."""
    import numpy as np
    planes = {n: eng.out[n][:, K - 1].detach().cpu().numpy().astype(np.float32) for n in sorted(eng.out)}
    total = sum(p.nbytes for p in planes.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES} byte limit"
    os.makedirs(out_dir, exist_ok=True)
    for n, p in planes.items():
        np.save(os.path.join(out_dir, f"{n}.npy"), p)


def time_mode(stepper, precision, forcing_names, prog, dist, dev, K, Wm, graph, world, rank, zero=False, engine_factory=None,
              dump_dir=None, stage_times=True):
    """One precision mode: K timed steps (barrier + sync on both sides, max over ranks) + per-stage HIP-event times.
    engine_factory(K, rank) -> engine: a stand-in engine (CPU test of the N > 1 orchestration); no stage timing then.
    dump_dir: rank 0 writes the outputs of the last timed step there (dump_outputs), after the timed region.
    stage_times: False (a plain run) skips the per-stage forwards and the host copies the CPU baseline compares against."""
    from ace_amd.distributed import AsyncEnsembleMean
    if engine_factory is not None:
        eng = engine_factory(K, rank)
        shape = (len(eng.out_names), *eng.out[eng.out_names[0]].shape[-2:])
        ens = AsyncEnsembleMean(shape, dev, dist)
        dt, allreduce_ms = timed_window(eng, ens, dist, dev, K, Wm, world)
        if dump_dir is not None and rank == 0:
            dump_outputs(eng, K, dump_dir)
        return dict(dt=dt, stages=None, x_cpu=None, y_gpu=None, allreduce_ms=allreduce_ms, allreduce_bytes=ens.buf.numel() * 4,
                    ensemble_mean=ens.result().clone())
    from ace_amd import _lib
    from ace_amd.rollout import RolloutEngine

    net = stepper.modules[0]
    net.set_precision(precision)
    T = K
    eng = RolloutEngine(stepper, batch=1, n_forward_steps=T, graph=None if graph == "none" else graph)
    g = torch.Generator().manual_seed(1 + rank)                   # member `rank`: its own initial state
    norm = stepper._step_obj.normalizer
    phys = lambda n, t: (t * float(norm.stds[n]) + float(norm.means[n])) if n in norm.means else t   # noqa: E731
    if zero:   # --zero-data: the normalised state is exactly zero as well
        phys = lambda n, t: (t * 0.0 + float(norm.means[n])) if n in norm.means else t * 0.0   # noqa: E731
    ic = {n: phys(n, torch.randn(1, 1, *IMG, generator=g)).to(dev) for n in prog}
    fc = {n: phys(n, torch.randn(1, T + 1, *IMG, generator=g)).to(dev) for n in list(forcing_names) + list(eng.target_names)}
    if "ocean_fraction" in fc:
        fc["ocean_fraction"] = torch.rand(1, T + 1, *IMG, generator=g).to(dev)
    eng.load(ic, fc)
    ens = AsyncEnsembleMean((len(eng.out_names), *IMG), dev, dist)   # side stream + events: the step stream never waits for RCCL
    dt, allreduce_ms = timed_window(eng, ens, dist, dev, K, Wm, world)
    if dump_dir is not None and rank == 0:
        dump_outputs(eng, K, dump_dir)

    stages = x_cpu = y_gpu = None
    if rank == 0 and stage_times:  # per-stage HIP-event timing of the forward, on the stream the kernels are launched on
        L = _lib.lib()
        ns = L.ace_sfno_num_stages()
        ms = (ctypes.c_float * ns)()
        calls = (ctypes.c_int * ns)()
        acc = [0.0] * ns
        reps = 5
        for _ in range(reps):
            _lib.check(L.ace_sfno_forward_timed(net._native, eng.x.data_ptr(), eng.y.data_ptr(), 1,
                                                _lib.current_stream(), ms, calls))
            for i in range(ns):
                acc[i] += ms[i] / reps
        model = stage_model(cin=len(stepper._step_obj.in_packer.names), cout=len(stepper._step_obj.out_packer.names))
        if precision == "fp32":   # exact-fp32 mode: the norm statistics are a stand-alone pass over the activation
            act_b = 384 * IMG[0] * IMG[1] * 4
            model["norm0_stats"] = model["norm1_stats"] = (3 * 384 * IMG[0] * IMG[1], act_b, act_b)
        stages = {}
        for i in range(ns):
            nm = L.ace_sfno_stage_name(i).decode()
            per_launch_ms = acc[i] / max(calls[i], 1)
            fl, by, moved = model[nm]
            # gbps: SURVEY 8(d)'s algorithmic bytes (dense operands) per launch time - the roofline convention; moved_gbps: the
            # bytes this build's layout actually transfers (triangular coefficients, folded table) - what the memory system sees
            stages[nm] = dict(ms_per_step=round(acc[i], 4), launches=calls[i], us_per_launch=round(per_launch_ms * 1e3, 2),
                              tflops=round(fl / per_launch_ms / 1e9, 2), gbps=round(by / per_launch_ms / 1e6, 1),
                              moved_bytes=int(moved), moved_gbps=round(moved / per_launch_ms / 1e6, 1))
        x_cpu = eng.x.detach().cpu()
        y_gpu = eng.y.detach().cpu()
    del eng
    torch.cuda.empty_cache()
    return dict(dt=dt, stages=stages, x_cpu=x_cpu, y_gpu=y_gpu, allreduce_ms=allreduce_ms, allreduce_bytes=ens.buf.numel() * 4)


# HBM bytes per launch and MFMA-busy from separate rocprofv3 --pmc passes (tools/pmc_collect.sh -> tools/pmc_to_profile.py ->
# profiles/r06_pmc_traffic.json).  FETCH_SIZE / WRITE_SIZE in KB; gfx950 correction: 16-byte-per-lane streaming reads are
# counted at half size (MI355X_MICROARCH.md "HBM").  The file carries the sha256 of the library the counters were taken on:
# figures are attached to the bench line ONLY when that is the library being timed now (otherwise null + the reason).
PMC_FILE = next((f for f in (os.path.join(ROOT, "profiles", n) for n in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json")) if os.path.exists(f)),
                os.path.join(ROOT, "profiles", "r06_pmc_traffic.json"))   # newest counter file; its build stamp decides whether it is used


def lib_sha256():
    import hashlib
    from ace_amd import _lib
    with open(_lib.LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def measured_counters():
    """{(mode, stage): entry} from PMC_FILE if it was taken on the library loaded now - the same binary, or one built from the
    same kernel sources and flags - else ({}, reason)."""
    try:
        with open(PMC_FILE) as f:
            d = json.load(f)
    except (OSError, ValueError):
        return {}, "no counter file (profiles/r06_pmc_traffic.json)"
    from ace_amd import build as _build
    if d.get("_lib_sha256") != lib_sha256() and d.get("_src_sha256") != _build.source_sha256():
        # neither the binary nor (hipcc output is not bit-reproducible: a rebuilt library differs) the kernel sources match
        return {}, (f"counter file is of another build (library sha256 {str(d.get('_lib_sha256'))[:12]} != timed {lib_sha256()[:12]}, "
                    f"kernel sources {str(d.get('_src_sha256'))[:12]} != {_build.source_sha256()[:12]})")
    return {tuple(k.split("|")): v for k, v in d.items() if not k.startswith("_") and isinstance(v, dict)}, None


# the kernel that runs each stage in the default (f16x3) mode
KERNEL_OF_STAGE = {
    "mlp.fc1": "conv_wl_kernel", "mlp.fc2+outer_skip": "conv_ws_kernel", "inner_skip+activation": "conv_ws_kernel",
    "dhconv": "dhconv_strip_kernel", "forward_transform.legendre": "legendre_fold_kernel",
    "inverse_transform.legendre": "legendre_fold_kernel", "forward_transform.dft": "dft_forward_fft_kernel",
    "inverse_transform.dft": "dft_inverse_fft_kernel", "encoder": "gemm4_f16x3_kernel + conv_ws_kernel", "decoder": "gemm3_f16x3_kernel",
}


def rooflines(main_mode, stages):
    """`roofline` (dominant kernel on its slowest stage) and `roofline_sht` (forward FFT + Legendre) from the per-stage event times"""
    model = stage_model()
    # dominant kernel = the kernel with the largest total time per step; it is reported on its slowest stage
    per_kernel = {}
    for st, v in stages.items():
        per_kernel[KERNEL_OF_STAGE.get(st, st)] = per_kernel.get(KERNEL_OF_STAGE.get(st, st), 0.0) + v["ms_per_step"]
    if main_mode == "fp32":
        dom = max(stages, key=lambda k: stages[k]["ms_per_step"])
    else:
        kdom = max(per_kernel, key=per_kernel.get)
        dom = max((st for st in stages if KERNEL_OF_STAGE.get(st, st) == kdom), key=lambda k: stages[k]["ms_per_step"])
    fl, by = model[dom][:2]
    t_launch = stages[dom]["us_per_launch"] * 1e-6
    pmc, pmc_note = measured_counters()
    ent = pmc.get((main_mode, dom), {})
    if main_mode == "fp32":   # exact-fp32 MFMA: the contraction kernels are bound by the fp32 matrix pipe
        roofline = dict(kernel=f"gemm_f32 engine ({dom})", bound="mfma", achieved=round(fl / t_launch / 1e12, 2),
                        peak=PEAK_MFMA_F32, unit="TFLOP/s", frac=round(fl / t_launch / 1e12 / PEAK_MFMA_F32, 4),
                        traffic=ent.get("bytes"), traffic_note=pmc_note)
    else:                     # compensated-fp16 MFMA (3 x 1/16 of the fp32 cost): HBM is the bounding roofline
        roofline = dict(kernel=f"{KERNEL_OF_STAGE.get(dom, dom)} ({dom})", bound="hbm", achieved=round(by / t_launch / 1e9, 1),
                        peak=PEAK_HBM, unit="GB/s", frac=round(by / t_launch / 1e9 / PEAK_HBM, 4),
                        traffic=ent.get("bytes"), traffic_note=pmc_note,
                        # north_star: MFMA-busy against the chip's peak.  Issue rate from the flop count (3 fp16 MFMAs per
                        # product) and, when the counters are of this build, SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x
                        # active cycles of one XCD)
                        mfma_f16_tflops=round(3 * fl / t_launch / 1e12, 1), mfma_f16_peak=2500.0,
                        mfma_busy_frac=round(3 * fl / t_launch / 1e12 / 2500.0, 4), mfma_busy_pmc=ent.get("mfma_busy"))
    sht_us = stages["forward_transform.dft"]["us_per_launch"] + stages["forward_transform.legendre"]["us_per_launch"]
    sht_bytes = 384 * 180 * 360 * 4 + 181 * 180 * 180 * 4 + 384 * 180 * 181 * 8     # 223.1 MB
    sht_moved = model["forward_transform.dft"][2] + model["forward_transform.legendre"][2] - 384 * 180 * 181 * 8   # X counted once each way
    roofline_sht = dict(kernel="forward SHT (dft_forward_fft_kernel + legendre_fold_kernel)", bound="hbm",
                        achieved=round(sht_bytes / (sht_us * 1e-6) / 1e9, 1), peak=PEAK_HBM, unit="GB/s",
                        frac=round(sht_bytes / (sht_us * 1e-6) / 1e9 / PEAK_HBM, 4),
                        moved_bytes_two_kernels=model["forward_transform.dft"][2] + model["forward_transform.legendre"][2],
                        traffic=(pmc[(main_mode, "forward_transform.dft")]["bytes"] +
                                 pmc[(main_mode, "forward_transform.legendre")]["bytes"])
                        if (main_mode, "forward_transform.dft") in pmc and
                           (main_mode, "forward_transform.legendre") in pmc else None, traffic_note=pmc_note)
    del sht_moved
    return roofline, roofline_sht


def extra_legs(stepper, forcing, prog, dist, dev, K, rank, hooks):
    """Two more legs of the same job, reported as extra keys: the one-year rollout BASELINE configs[1] names (1460
    six-hourly steps as 1460 / K windows chained through the engine's state feedback, per-step hipGraph) and the "S80" state
    (8 forcing + 36 prognostic in = 44, 36 prognostic + 36 diagnostic out = 72 channels; the headline state is ACE2's 44 / 50)."""
    from ace_amd.rollout import RolloutEngine
    out = {}
    # ---- 1460 steps: windows of K steps, the last state of a window is the next one's initial condition
    eng = RolloutEngine(stepper, batch=1, n_forward_steps=K, graph="step")
    g = torch.Generator().manual_seed(1 + rank)
    norm = stepper._step_obj.normalizer
    phys = lambda n, t: (t * float(norm.stds[n]) + float(norm.means[n])) if n in norm.means else t   # noqa: E731
    ic = {n: phys(n, torch.randn(1, 1, *IMG, generator=g)).to(dev) for n in prog}
    fc = {n: phys(n, torch.randn(1, K + 1, *IMG, generator=g)).to(dev) for n in list(forcing) + list(eng.target_names)}
    if "ocean_fraction" in fc:
        fc["ocean_fraction"] = torch.rand(1, K + 1, *IMG, generator=g).to(dev)
    eng.load(ic, fc)
    n_year, done = 1460, 0
    with torch.no_grad():
        eng.run_window()                                          # untimed: graph capture
        eng.load(ic, fc)
        _sync(dev)
        t0 = time.perf_counter()
        while done < n_year:
            n = min(K, n_year - done)
            for s_ in range(n):
                eng._enqueue_step(s_, True)
            done += n
            if done < n_year:
                for nme in eng.prognostic:                         # (continue_from_last, for a possibly partial last window)
                    eng.ic[nme].copy_(eng.out[nme][:, n - 1:n])
        _sync(dev)
        dt = time.perf_counter() - t0
    last = torch.stack([eng.out[nme][0, (n_year - 1) % K] for nme in eng.out_names])
    out["one_year_rollout"] = {"steps": n_year, "seconds": round(dt, 3), "steps_per_s": round(n_year / dt, 2),
                               "ms_per_step": round(dt / n_year * 1e3, 4), "graph": "step", "windows_of": K,
                               "final_state_finite": bool(torch.isfinite(last).all()),
                               "final_state_absmax": float(last.abs().max()),
                               "simulated_years_per_day": round(86400.0 / dt, 1)}
    del eng
    if hooks:
        return out
    # ---- S80: the same network body with 72 output channels
    import ace_amd
    from ace_amd.step import NormalizationConfig
    f80 = [f"forcing_{i}" for i in range(8)]
    p80 = [f"prog_{i}" for i in range(36)]
    d80 = [f"diag_{i}" for i in range(36)]
    cfg = ace_amd.SingleModuleStepConfig(
        builder=ace_amd.ModuleSelector(type="SphericalFourierNeuralOperatorNet", config=ACE2),
        in_names=f80 + p80, out_names=p80 + d80,
        normalization=NormalizationConfig(means={k: 0.1 for k in f80 + p80 + d80}, stds={k: 1.1 for k in f80 + p80 + d80}))
    torch.manual_seed(0)
    st80 = ace_amd.Stepper.from_config(cfg, ace_amd.DatasetInfo(IMG), device=dev)
    st80.set_eval()
    r80 = time_mode(st80, stepper.modules[0].precision if hasattr(stepper.modules[0], "precision") else "f16x3", f80, p80, dist, dev,
                    K, 2, "step", 1, rank)
    out["state_s80"] = {"in_channels": 44, "out_channels": 72, "steps_per_s": round(K / r80["dt"], 3),
                        "ms_per_step": round(r80["dt"] / K * 1e3, 4),
                        "decoder_us": r80["stages"]["decoder"]["us_per_launch"] if r80["stages"] else None}
    del st80
    torch.cuda.empty_cache()
    return out


def main(argv=None, engine_factory=None, device=None):
    """engine_factory / device: the CPU test of the rank orchestration (tests/test_bench_ranks_cpu.py) passes a stand-in engine
    and "cpu"; everything below - argument checks, the distributed facade, warm-up, timed region, max over ranks, the gather of
    the per-rank records and the JSON line - is then the code `bench.py --gpus N` runs on the devices."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graph", default="step", choices=["none", "step", "window"])
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the second precision mode, per-stage HIP-event times and rooflines, "
                         "the CPU baseline and the extra legs")
    ap.add_argument("--precision", default="both", choices=["both", "f16x3", "fp32"],
                    help="'both': the default (f16x3) is the headline; with --full the exact-fp32 arithmetic is timed in the same run")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra-legs", action="store_true", help="with --full: skip the 1460-step and the S80 (44 in / 72 out) legs")
    ap.add_argument("--zero-data", action="store_true",
                    help="DIAGNOSTIC (DVFS give-back check, MI355X_MICROARCH.md): all weights and all inputs zero - same kernels, same "
                         "instruction streams, no operand switching; the line is marked invalid as a result")
    ap.add_argument("--hooks", action="store_true",
                    help="ACE2-style post-step physics (atmosphere corrector + prescribed-SST ocean) inside the timed loop")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the output fields of the last timed step of the headline mode as DIR/<name>.npy "
                         "(float32); weights and inputs are seeded, so two builds can be compared field by field")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    from ace_amd.distributed import Distributed
    from ace_amd.sfno import DEFAULT_PRECISION

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        assert world == 1, f"--gpus {args.gpus} but WORLD_SIZE={world}"
        assert args.gpus == 1, "launch with torch.distributed.run for --gpus > 1"
    if engine_factory is None:
        assert torch.cuda.is_available(), "bench.py needs an MI355X"
        ndev = torch.cuda.device_count()
        if local_rank >= ndev and os.environ.get("ACE_DIST_BACKEND") != "gloo":
            raise SystemExit(f"LOCAL_RANK {local_rank} but {ndev} device(s): one rank per GPU (ACE_DIST_BACKEND=gloo lets ranks share "
                             "devices for a pre-flight of the N > 1 path without RCCL)")
        torch.cuda.set_device(local_rank % ndev)
        dev = torch.device("cuda", local_rank % ndev)
    else:
        dev = torch.device(device or "cpu")
    dist = Distributed.get_instance()

    K, Wm = args.steps, args.warmup
    stepper = forcing = prog = None
    if engine_factory is None:
        stepper, forcing, prog, _diag = build_stepper(dev, seed=0, hooks=args.hooks)   # same weights on every rank (one model, N members)
        if args.zero_data:
            with torch.no_grad():
                for p_ in stepper.modules[0].parameters():
                    p_.zero_()
    modes = [DEFAULT_PRECISION] + (["fp32" if DEFAULT_PRECISION != "fp32" else "f16x3"] if args.precision == "both" else [])
    if args.precision in ("f16x3", "fp32"):
        modes = [args.precision]
    if engine_factory is not None or not args.full:
        modes = modes[:1]
    runs = {m: time_mode(stepper, m, forcing, prog, dist, dev, K, Wm, args.graph, world, rank, zero=args.zero_data,
                         engine_factory=engine_factory, dump_dir=args.dump_outputs if m == modes[0] else None,
                         stage_times=args.full) for m in modes}
    ranks_info = gather_rank_records(dist, dev, rank, local_rank, world, runs[modes[0]]["allreduce_ms"])

    result = None
    if rank == 0:
        main_mode = modes[0]
        r = runs[main_mode]
        stages = r["stages"]
        roofline = roofline_sht = cpu = None
        if stages is not None:
            roofline, roofline_sht = rooflines(main_mode, stages)
        if stages is not None and not args.no_cpu_baseline and world == 1:   # the CPU baseline is a single-GPU-run leg (rank 0 at N = 1 only)
            cpu, y_cpu = cpu_baseline(stepper, r["x_cpu"])
            cpu["parity_rel_err_vs_gpu"] = {m: float((runs[m]["y_gpu"] - y_cpu).abs().max() / y_cpu.abs().max()) for m in modes}
        steps_per_s = world * K / r["dt"]
        dtype = {"fp32": "f32", "f16x3": "f32 (contractions with K>=32 on error-compensated fp16x3 MFMA, fp32 accumulate; "
                                         "DFT, norms, epilogues fp32; measured error vs fp64 below the fp32 CPU reference's)"}
        result = {
            "metric": "rollout steps/sec (6-hourly forward steps of the 1-degree SFNO, whole job)",
            "value": round(steps_per_s, 3), "unit": "steps/s", "n_gpus": world, "steps": K, "warmup": Wm,
            "ms_per_step": round(r["dt"] / K * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": dtype[main_mode],
            "data": "synthetic" if not args.zero_data else "ALL-ZERO weights and state (--zero-data diagnostic; not a result)",
            "simulated_years_per_day": round(steps_per_s * 86400 / 1460, 1),
            "config": {"workload": "ACE2-ERA5-shape 1deg SFNO rollout (BASELINE.json configs[1]): embed 384, 8 layers, "
                                   "dhconv, 44 in / 50 out channels, 180x360 legendre-gauss, lmax 180, mmax 181, "
                                   "B=1 member per GPU, random-init weights",
                       "members": world, "members_per_gpu": 1, "graph": args.graph, "precision": main_mode,
                       "collective": "RCCL all-reduce mean of the (50,180,360) output state once per window" if world > 1 else "none"},
            "roofline": roofline, "roofline_sht": roofline_sht, "stages": stages, "cpu_baseline": cpu,
            "lib_sha256": lib_sha256() if engine_factory is None else None,
            "multi_gpu": multi_gpu_block(world, ranks_info, r["allreduce_bytes"]),
        }
        for m in modes[1:]:
            result[f"mode_{m}"] = {"value": round(world * K / runs[m]["dt"], 3), "unit": "steps/s",
                                   "ms_per_step": round(runs[m]["dt"] / K * 1e3, 4), "stages": runs[m]["stages"]}
    if engine_factory is None and world == 1 and args.full and not args.no_extra_legs and not args.zero_data:
        stepper.modules[0].set_precision(modes[0])
        try:
            legs = extra_legs(stepper, forcing, prog, dist, dev, K, rank, args.hooks)
        except Exception as e:   # the headline line must not depend on an extra leg
            legs = {"extra_legs_error": f"{type(e).__name__}: {e}"}
        if result is not None:
            result.update(legs)
    dist.barrier()
    if rank == 0:
        print(json.dumps(result), flush=True)
    dist.shutdown()
    return result if rank == 0 else runs[modes[0]]


if __name__ == "__main__":
    main()
