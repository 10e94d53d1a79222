"""ctypes binding of the C ABI in include/lfsd_cpdp.h + the hipcc build of one model library.

PyTorch is plumbing here: tensors own the HBM buffers and the HIP stream; every
numeric step of the hot path runs in the model's shared library.  There is no
CPU fallback: a missing library is built with hipcc or the call fails loudly.
"""
import ctypes
import os
import shutil
import subprocess

import torch

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.join(PKG_DIR, "csrc")
GEN_DIR = os.path.join(CSRC_DIR, "gen")
BUILD_DIR = os.path.join(CSRC_DIR, "build")
INCLUDE_DIR = os.path.join(os.path.dirname(PKG_DIR), "include")

LFSD_F32, LFSD_F64 = 0, 1
STATUS = {1: "converged", 2: "stalled", 3: "maxiter", 4: "failed"}
OPT_METHODS = {"Vanilla": 0, "Nesterov": 1, "Adam": 2, "Nadam": 3, "AMSGrad": 4, "LM": 5}
MAPPINGS = {"auto": 0, "lockstep": 1, "wide": 2}


class LfsdError(RuntimeError):
    pass


class _ModelInfo(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int), ("n_state", ctypes.c_int), ("n_control", ctypes.c_int),
                ("n_auxvar", ctypes.c_int), ("n_const", ctypes.c_int), ("time_varying", ctypes.c_int),
                ("lanes_per_trajectory", ctypes.c_int), ("is_emulator", ctypes.c_int),
                ("name", ctypes.c_char_p), ("hash", ctypes.c_char_p)]


def lanes_for(n, m, p):
    need = max(n + m, n + p, 8)
    g = 8
    while g < need:
        g *= 2
    if g > 64:
        raise LfsdError("model too wide for one wavefront per trajectory: n+max(m,p) = %d > 64" % need)
    return g


def find_hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise LfsdError("hipcc not found: the HIP model library cannot be built")


def library_path(model_hash):
    return os.path.join(BUILD_DIR, "liblfsd_%s.so" % model_hash)


def header_path(model_hash):
    return os.path.join(GEN_DIR, "%s.h" % model_hash)


def write_header(spec, force=False):
    from . import codegen
    os.makedirs(GEN_DIR, exist_ok=True)
    hp = header_path(spec.hash())
    if force or not os.path.exists(hp):
        src = codegen.emit_header(spec)
        tmp = hp + ".tmp%d" % os.getpid()
        with open(tmp, "w") as f:
            f.write(src)
        os.replace(tmp, hp)
    return hp


def _hipcc_flags(spec, extra=()):
    g = lanes_for(spec.n, spec.m, spec.p)
    return [find_hipcc(), "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O3", "-fPIC",
            "-fno-signed-zeros", "-fvisibility=hidden",
            "-DLFSD_G=%d" % g, '-DLFSD_MODEL_HEADER="gen/%s.h"' % spec.hash(), "-I" + CSRC_DIR] + list(extra)


# Per translation unit.  Rounds 1-5 compiled the first unit with `-mllvm -amdgpu-sched-strategy=max-ilp` (round 1: 5 % off oc_solve;
# the Riccati sweep lost 25 % with it, hence its own unit).  Round 6 dropped it: two builds of the wide OC kernel were WRONG under
# that scheduler and right under the default one with the same source (profiles/r06_f_wide_stale_cost.txt), and it no longer pays:
# headline 966 300 -> 966 700 it/s, rocket step 40.8 -> 38.8 ms, robot arm 15.31 -> 15.41 ms, fp64 headline 13.5 -> 13.9 ms
# (profiles/r06_i_max_ilp_ab.txt).  The cause turned out to be independent of the scheduler -- VGPR spills placed before the exec restore
# of a join block, which a third wrong build showed under the DEFAULT one -- and every build is now scanned for it (_checked_build below).
TUNED_CAPI = ()
TUNED_RICCATI = ()
TUNED_CUBIC = ()
UNITS = ("capi", "riccati", "cubic")


def hipcc_commands(spec, out, extra=(), extra_capi=TUNED_CAPI, extra_riccati=TUNED_RICCATI, extra_cubic=TUNED_CUBIC):
    """Product build: three translation units (UNITS) -- the Riccati sweep apart from everything else, so that each gets the
    compiler settings it measured best with (csrc/lfsd_internal.h, profiles/r01_tune_compiler_flags.txt), and the kernels of
    interpolation level 2 apart from both, so that the device code of the first two is what it was without them (csrc/
    lfsd_cubic.inc) -- then the link.  All are compiled without clang's SLP vectoriser.  Returns (one command per unit + the
    link command, the object files)."""
    flags = _hipcc_flags(spec, extra) + ["-fno-slp-vectorize"]
    o1, o2, o3 = out + ".capi.o", out + ".riccati.o", out + ".cubic.o"
    return ([flags + ["-c", "-DLFSD_SPLIT_RICCATI", os.path.join(CSRC_DIR, "lfsd_capi.cpp"), "-o", o1] + list(extra_capi),
             flags + ["-c", os.path.join(CSRC_DIR, "lfsd_riccati.cpp"), "-o", o2] + list(extra_riccati),
             flags + ["-c", os.path.join(CSRC_DIR, "lfsd_cubic.cpp"), "-o", o3] + list(extra_cubic),
             [find_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", o1, o2, o3, "-o", out]], [o1, o2, o3])


# every hand-written file a model library is compiled from (rebuild when any of them is newer than the .so)
KERNEL_SOURCES = ("cpdp_kernels.h", "cpdp_common.h", "cpdp_oc.h", "cpdp_aux.h", "cpdp_opt.h", "cpdp_rows.h", "cpdp_spline.h", "cpdp_sample.h", "cpdp_lm.h", "cpdp_groups.h", "cpdp_times.h", "cpdp_lm_times.h", "cpdp_aux_sweeps.inc", "lfsd_capi.cpp",
                  "lfsd_internal.h", "lfsd_riccati.inc", "lfsd_riccati.cpp", "lfsd_cubic.inc", "lfsd_cubic.cpp")


# Every build is compiled with -save-temps and its gfx950 assembly scanned by lfsd_amd.isa_check (VGPR spills placed before the
# exec restore of a join block: two wrong builds of the wide OC kernel in round 6 -- isa_check.py, profiles/
# r06_v_spill_before_exec_restore.txt).  A translation unit whose assembly shows the pattern is recompiled with the next entry of
# this list -- other instruction schedulers: the placement moves with any perturbation of the kernel -- until the scan is clean;
# if none is, the build FAILS (no library is better than a library whose upper lanes read stale spill slots).
SCHEDULE_ALTERNATES = ((), ("-mllvm", "-amdgpu-sched-strategy=max-ilp"), ("-mllvm", "-amdgpu-sched-strategy=max-memory-clause"),
                       ("-mllvm", "-amdgpu-use-amdgpu-trackers"), ("-mllvm", "-greedy-reverse-local-assignment"))
# The same scan rejects a build in which a DPP instruction -- the hand-written v_fmac_f32_dpp of cpdp_common.h's fmac2_row_bcast above
# all: the compiler's hazard recognizer does not look into an asm statement -- has too few wait states behind a vector instruction
# that wrote its src0 or EXEC (isa_check.find_dpp_hazards): where the register allocator puts a copy-back is nothing the source controls.
ISA_CHECK_VERSION = 4      # (2: loop exits without a skip branch are examined too; 3: the entries of else-regions count as restores;
                           #  4: wait states in front of DPP instructions)


def isa_record_path(lib_path):
    return lib_path + ".isa.json"


def isa_record_clean(lib_path):
    """The library was built by _checked_build of this version and every unit passed (a library without such a record -- built by an
    older tree or by hand -- counts as stale: build_library compiles it again)."""
    import json
    try:
        rec = json.load(open(isa_record_path(lib_path)))
    except (OSError, ValueError):
        return False
    units = rec.get("units", {})
    return rec.get("isa_check") == ISA_CHECK_VERSION and set(units) == set(UNITS) and all(u.get("hazards") == 0 for u in units.values()) \
        and rec.get("sha256") == _sha256(lib_path)      # (the record belongs to THIS file, not to one a later hand build replaced)


def _sha256(path):
    import hashlib
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def _checked_build(spec, out, extra=(), verbose=False, what="model"):
    """Compile the translation units (UNITS) into `out` (csrc/build/...), each with the first entry of SCHEDULE_ALTERNATES whose device
    assembly passes isa_check; writes `<out>.isa.json` (what was scanned, which flags each unit was built with).  Raises LfsdError."""
    import json, shutil, tempfile
    from . import isa_check
    os.makedirs(BUILD_DIR, exist_ok=True)
    work = tempfile.mkdtemp(prefix="obj%d_" % os.getpid(), dir=BUILD_DIR)
    try:
        tmp = os.path.join(work, "lib.so")
        record = {"isa_check": ISA_CHECK_VERSION, "units": {}}
        objs = []
        for ui, unit in enumerate(UNITS):
            tuned = (TUNED_CAPI, TUNED_RICCATI, TUNED_CUBIC)[ui]
            tried, built = [], False
            for alt in SCHEDULE_ALTERNATES:
                kw = {"extra_" + unit: tuple(tuned) + tuple(alt)}
                cmds, obj_paths = hipcc_commands(spec, tmp, list(extra), **kw)
                cmd = cmds[ui] + ["-save-temps=obj"]
                if verbose:
                    print(" ".join(cmd))
                for f in os.listdir(work):      # (the temporaries of the previous attempt)
                    if f.endswith(".s"):
                        os.remove(os.path.join(work, f))
                r = subprocess.run(cmd, cwd=CSRC_DIR, capture_output=True, text=True)
                if r.returncode != 0:
                    if alt:      # a toolchain that does not know this -mllvm option: next
                        tried.append({"flags": list(alt), "error": r.stderr[-300:]})
                        continue
                    raise LfsdError("hipcc failed for %s %s:\n%s\n%s" % (what, spec.name, r.stdout[-4000:], r.stderr[-4000:]))
                asm = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
                if len(asm) != 1:
                    raise LfsdError("no device assembly to check for %s %s (%s): %s" % (what, spec.name, unit, sorted(os.listdir(work))))
                text = open(os.path.join(work, asm[0])).read()
                hz = isa_check.find_exec_hazards(text) + isa_check.find_dpp_hazards(text)
                if hz:
                    tried.append({"flags": list(alt), "hazards": len(hz), "first": hz[0]})
                    if verbose:
                        print("isa_check: %d spill(s) before an exec restore / DPP instruction(s) too close to a writer in %s (%s, flags %s): %s" % (len(hz), spec.name, unit, list(alt), hz[0]))
                    continue
                record["units"][unit] = dict(isa_check.summary(text), dpp=isa_check.dpp_count(text), flags=list(tuned) + list(alt), hazards=0, rejected=tried)
                objs.append(obj_paths[ui])
                built = True
                break
            if not built:
                raise LfsdError("every build of %s %s (%s) has VGPR spills before an exec restore or a DPP instruction too close to a writer (lfsd_amd/isa_check.py): %s"
                                % (what, spec.name, unit, tried))
        link = hipcc_commands(spec, tmp, list(extra))[0][-1]
        r = subprocess.run(link, cwd=CSRC_DIR, capture_output=True, text=True)
        if r.returncode != 0:
            raise LfsdError("link failed for %s %s:\n%s" % (what, spec.name, r.stderr[-3000:]))
        record["sha256"] = _sha256(tmp)
        with open(isa_record_path(out) + ".tmp%d" % os.getpid(), "w") as f:
            json.dump(record, f, indent=1, sort_keys=True, default=str)
        os.replace(tmp, out)
        os.replace(isa_record_path(out) + ".tmp%d" % os.getpid(), isa_record_path(out))
        return record
    finally:
        shutil.rmtree(work, ignore_errors=True)


def build_library(spec, force=False, verbose=False):
    """Generate the model header and compile the gfx950 shared library in-tree (csrc/build/), assembly checked (above)."""
    os.makedirs(BUILD_DIR, exist_ok=True)
    out = library_path(spec.hash())
    write_header(spec, force=force)
    deps = [header_path(spec.hash()), os.path.join(INCLUDE_DIR, "lfsd_cpdp.h")] + \
        [os.path.join(CSRC_DIR, f) for f in KERNEL_SOURCES]
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps) and isa_record_clean(out):
        return out
    _checked_build(spec, out, verbose=verbose)
    return out


def variant_library_path(spec, tag):
    return os.path.join(BUILD_DIR, "ab_%s_%s.so" % (spec.hash(), tag))


def build_variant_library(spec, tag, flags):
    """hipcc build of a VARIANT of a model library (build switches of csrc/cpdp_common.h set on the command line) into
    csrc/build/ab_<hash>_<tag>.so, rebuilt when a kernel source is newer.  The A/B tests of the GPU tier compare the product
    build with such variants; never loaded by the product path.  Same assembly check as the product build."""
    write_header(spec)
    out = variant_library_path(spec, tag)
    deps = [header_path(spec.hash())] + [os.path.join(CSRC_DIR, f) for f in KERNEL_SOURCES]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(p) for p in deps) and isa_record_clean(out):
        return out
    _checked_build(spec, out, extra=list(flags), what="variant %s of model" % tag)
    return out


# build variants the -m gpu tier compares the product with: (model kind, n_grid, tag, flags).  "plain" = every schedule off.
PLAIN_SCHEDULE = ("-DLFSD_LEAN_TC=1", "-DLFSD_COARSE_START=0", "-DLFSD_COARSE_TIME=1", "-DLFSD_MS=0")
GPU_TIER_VARIANTS = (("quadrotor", 50, "nocoarse", ("-DLFSD_COARSE_START=0",)),
                     ("quadrotor", 50, "plain", PLAIN_SCHEDULE), ("cartpole", 40, "plain", PLAIN_SCHEDULE),
                     ("rocket", 40, "plain", PLAIN_SCHEDULE), ("robotarm", 50, "plain", PLAIN_SCHEDULE),
                     # the Riccati sweep with one staging pass per split unit (tests/test_riccati_pair_stage_gpu.py)
                     ("quadrotor", 50, "ricpair0", ("-DLFSD_RIC_PAIR_STAGE=0",)),
                     # the lean fp32 OC kernel with its group hand-overs through LDS (tests/test_oc_dpp_xchg_gpu.py)
                     ("quadrotor", 50, "ocdpp0", ("-DLFSD_OC_DPP_XCHG=0",)), ("rocket", 40, "ocdpp0", ("-DLFSD_OC_DPP_XCHG=0",)))


def build_gpu_tier_variants(verbose=False):
    """Prebuild the variants above so that they travel with the tree (optional: a failure here is reported, not raised --
    the product libraries do not depend on them)."""
    from concurrent.futures import ThreadPoolExecutor
    from . import models
    built = {}
    with ThreadPoolExecutor(max_workers=max(1, min(4, (os.cpu_count() or 2) // 2))) as pool:
        futs = {}
        for kind, n_grid, tag, flags in GPU_TIER_VARIANTS:
            oc = models.ZOO[kind](n_grid=n_grid)[0]
            futs[(kind, tag)] = pool.submit(build_variant_library, oc.model_spec(), tag, flags)
        for (kind, tag), fut in futs.items():
            try:
                built[(kind, tag)] = fut.result()
                if verbose:
                    print("variant", kind, tag, built[(kind, tag)])
            except Exception as exc:      # noqa: BLE001
                print("WARNING: test variant %s/%s not built: %s" % (kind, tag, str(exc)[:300]))
    return built


_DT = {torch.float32: LFSD_F32, torch.float64: LFSD_F64}


class ModelLibrary:
    """One loaded model library (all entry points of include/lfsd_cpdp.h)."""

    EXPORTS = ("lfsd_get_model_info", "lfsd_interface_dim", "lfsd_const_default", "lfsd_coc_workspace_bytes", "lfsd_coc_solve",
               "lfsd_aux_solve", "lfsd_aux_riccati", "lfsd_aux_forward", "lfsd_optimizer_step", "lfsd_lookahead",
               "lfsd_stop_compact", "lfsd_gather_rows", "lfsd_scatter_rows", "lfsd_grid_curvature", "lfsd_aux_solve_cubic",
               "lfsd_aux_riccati_cubic", "lfsd_aux_forward_cubic", "lfsd_sample_grid", "lfsd_waypoint_vjp",
               "lfsd_optimizer_step_rows", "lfsd_lookahead_rows", "lfsd_trace_append", "lfsd_normal_matrix", "lfsd_lm_step",
               "lfsd_group_reduce", "lfsd_aux_forward_weighted", "lfsd_aux_forward_cubic_weighted", "lfsd_normal_matrix_weighted",
               "lfsd_waypoint_time_grad", "lfsd_tau_project", "lfsd_time_normal_blocks", "lfsd_lm_step_times")

    def __init__(self, path):
        if not os.path.exists(path):
            raise LfsdError("model library %s does not exist (build it with __graft_entry__.build() or "
                            "COCSys.compile())" % path)
        self.path = path
        self.lib = ctypes.CDLL(path)
        for sym in self.EXPORTS:
            if not hasattr(self.lib, sym):
                raise LfsdError("%s does not export %s" % (path, sym))
        L = self.lib
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.lfsd_get_model_info.argtypes = [ctypes.POINTER(_ModelInfo)]
        L.lfsd_const_default.argtypes = [ci]
        L.lfsd_const_default.restype = cd
        L.lfsd_coc_workspace_bytes.argtypes = [ci, ci, ci, ci, ci, ci]
        L.lfsd_coc_workspace_bytes.restype = ctypes.c_size_t
        L.lfsd_coc_solve.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, cd, vp, vp, vp, vp, vp, vp, ci, cd, ci,
                                     ci, vp, ctypes.c_size_t, vp]
        L.lfsd_aux_solve.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp,
                                     ci, cd, vp, vp, ci, vp]
        L.lfsd_aux_riccati.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, cd, vp, vp, ci, vp]
        L.lfsd_aux_forward.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp,
                                       ci, cd, vp, vp, ci, vp]
        L.lfsd_grid_curvature.argtypes = [ci, ci, ci, ci, vp, vp, vp]
        L.lfsd_aux_solve_cubic.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp,
                                           ci, cd, vp, vp, ci, vp]
        L.lfsd_aux_riccati_cubic.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, cd, vp, vp, ci, vp]
        L.lfsd_aux_forward_cubic.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp,
                                             ci, cd, vp, vp, ci, vp]
        L.lfsd_sample_grid.argtypes = [ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
        L.lfsd_waypoint_vjp.argtypes = [ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        L.lfsd_optimizer_step.argtypes = [ci, ci, ci, ci, ci, cd, cd, cd, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp]
        L.lfsd_lookahead.argtypes = [ci, ctypes.c_longlong, cd, vp, vp, vp, vp]
        L.lfsd_optimizer_step_rows.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.lfsd_lookahead_rows.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp]
        L.lfsd_trace_append.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        L.lfsd_normal_matrix.argtypes = [ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
        L.lfsd_lm_step.argtypes = [ci, ci, ci, cd, cd, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        # (ABI 16: wp_weight after waypoints / after taus)
        L.lfsd_aux_forward_weighted.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp,
                                                ci, cd, vp, vp, ci, vp]
        L.lfsd_aux_forward_cubic_weighted.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp,
                                                      vp, vp, ci, cd, vp, vp, ci, vp]
        L.lfsd_normal_matrix_weighted.argtypes = [ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        L.lfsd_group_reduce.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        # (ABI 17: learnable waypoint times)
        L.lfsd_waypoint_time_grad.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, cd, vp, vp]
        L.lfsd_tau_project.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, cd, vp, vp]
        # (ABI 18: Levenberg-Marquardt over parameters and waypoint times jointly)
        L.lfsd_time_normal_blocks.argtypes = [ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.lfsd_lm_step_times.argtypes = [ci, ci, ci, ci, ci, cd, cd, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                         vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.lfsd_stop_compact.argtypes = [ci, ci, ci, vp, vp, vp, vp, cd, cd, ci, vp, vp, vp, vp, vp, vp]
        L.lfsd_gather_rows.argtypes = [ci, ctypes.c_longlong, vp, vp, vp, vp]
        L.lfsd_scatter_rows.argtypes = [ci, ctypes.c_longlong, vp, vp, vp, vp]
        info = _ModelInfo()
        rc = L.lfsd_get_model_info(ctypes.byref(info))
        if rc != 0 or info.abi_version != 18:
            raise LfsdError("ABI mismatch in %s" % path)
        self.n_state, self.n_control, self.n_auxvar, self.n_const = (info.n_state, info.n_control, info.n_auxvar,
                                                                      info.n_const)
        self.time_varying = bool(info.time_varying)
        self.lanes = info.lanes_per_trajectory
        self.is_emulator = bool(info.is_emulator)
        self.name = info.name.decode()
        self.hash = info.hash.decode()
        self.const_defaults = [L.lfsd_const_default(i) for i in range(self.n_const)]
        self.n_interface = int(L.lfsd_interface_dim())      # outputs of the compiled interface function (0: none)

    # ---- argument plumbing ---------------------------------------------------------------
    def _check(self, t, shape, dtype, name, optional=False):
        if t is None:
            if optional:
                return None
            raise LfsdError("%s is required" % name)
        if not isinstance(t, torch.Tensor):
            raise LfsdError("%s must be a torch tensor" % name)
        if tuple(t.shape) != tuple(shape):
            raise LfsdError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
        if t.dtype != dtype:
            raise LfsdError("%s has dtype %s, expected %s" % (name, t.dtype, dtype))
        if not t.is_contiguous():
            raise LfsdError("%s must be contiguous" % name)
        if self.is_emulator:
            if t.device.type != "cpu":
                raise LfsdError("the SIMT-emulator test library only takes CPU tensors (%s)" % name)
        elif t.device.type != "cuda":
            raise LfsdError("%s lives on %s: the HIP library needs device memory (no CPU fallback)" % (name, t.device))
        return t

    @staticmethod
    def _p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def _stream(self, ref):
        if self.is_emulator:
            return None
        return ctypes.c_void_p(torch.cuda.current_stream(ref.device).cuda_stream)

    def _on(self, ref):
        """Context that makes the tensors' GPU the current HIP device (kernel launches go to the current device)."""
        import contextlib
        return contextlib.nullcontext() if self.is_emulator else torch.cuda.device(ref.device)

    @staticmethod
    def _rc(rc, what):
        if rc != 0:
            raise LfsdError("%s failed with code %d" % (what, rc))

    # ---- entry points ----------------------------------------------------------------------
    def coc_workspace_bytes(self, dtype, batch, n_grid, exact_after=16, mapping="auto", bounded=False):
        return int(self.lib.lfsd_coc_workspace_bytes(_DT[dtype], batch, n_grid, int(exact_after), MAPPINGS[mapping],
                                                      1 if bounded else 0))

    def coc_solve(self, ini_state, horizon, auxvar, consts, n_grid, steps_per_grid=4, u_init=None, max_iter=100,
                  tol=None, workspace=None, out=None, exact_after=16, control_lb=None, control_ub=None, mapping="auto",
                  state_lb=None, state_ub=None, state_mult=None, state_rho=0.0):
        """state_lb / state_ub [n], state_mult [B][n_grid][2][n], state_rho: ONE augmented-Lagrangian subproblem of the
        state-bounded NLP (include/lfsd_cpdp.h); the multiplier loop is COCSys.cocSolverBatch."""
        dt = ini_state.dtype
        B = ini_state.shape[0]
        n, m, p, nc = self.n_state, self.n_control, self.n_auxvar, self.n_const
        self._check(ini_state, (B, n), dt, "ini_state")
        self._check(horizon, (B,), dt, "horizon")
        self._check(auxvar, (B, p), dt, "auxvar")
        per_traj = 0
        if nc:
            if consts is None:
                raise LfsdError("consts is required (n_const=%d)" % nc)
            if consts.dim() == 2:
                self._check(consts, (B, nc), dt, "consts")
                per_traj = 1
            else:
                self._check(consts, (nc,), dt, "consts")
        else:
            consts = None
        self._check(u_init, (B, n_grid, m), dt, "u_init", optional=True)
        self._check(control_lb, (m,), dt, "control_lb", optional=True)
        self._check(control_ub, (m,), dt, "control_ub", optional=True)
        if (control_lb is None) != (control_ub is None):
            raise LfsdError("control_lb and control_ub go together")
        if state_lb is not None:
            self._check(state_lb, (n,), dt, "state_lb")
            self._check(state_ub, (n,), dt, "state_ub")
            self._check(state_mult, (B, n_grid, 2, n), dt, "state_mult")
            if control_lb is None:
                raise LfsdError("state bounds need the control-bound arrays beside them (+-1e20 where there is none)")
        dev = ini_state.device
        if out is None:
            out = dict(state_grid=torch.empty((B, n_grid + 1, n), dtype=dt, device=dev),
                       control_grid=torch.empty((B, n_grid + 1, m), dtype=dt, device=dev),
                       costate_grid=torch.empty((B, n_grid + 1, n), dtype=dt, device=dev),
                       cost=torch.empty((B,), dtype=dt, device=dev),
                       iters=torch.zeros((B,), dtype=torch.int32, device=dev),
                       status=torch.zeros((B,), dtype=torch.int32, device=dev))
        need = self.coc_workspace_bytes(dt, B, n_grid, exact_after, mapping, control_lb is not None)
        if workspace is None or workspace.numel() * workspace.element_size() < need:
            workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        if tol is None:
            tol = 1e-6 if dt == torch.float32 else 1e-9
        args = (_DT[dt], B, n_grid, steps_per_grid, self._p(ini_state), self._p(horizon), self._p(auxvar),
                self._p(consts), per_traj, self._p(u_init), self._p(control_lb), self._p(control_ub),
                self._p(state_lb), self._p(state_ub), self._p(state_mult), float(state_rho),
                self._p(out["state_grid"]), self._p(out["control_grid"]),
                self._p(out["costate_grid"]), self._p(out["cost"]), self._p(out["iters"]), self._p(out["status"]),
                int(max_iter), float(tol), int(exact_after), MAPPINGS[mapping], self._p(workspace),
                workspace.numel() * workspace.element_size(), self._stream(ini_state))
        with self._on(ini_state):
            self._rc(self.lib.lfsd_coc_solve(*args), "lfsd_coc_solve")
        out["workspace"] = workspace
        return out

    def grid_curvature(self, grid, out=None):
        """Curvature grid c_k = h^2 y''(t_k) / 6 of the not-a-knot cubic spline (scipy's interp1d(kind='cubic'), CPDP.py:388-390)
        through every component of ``grid`` [B, n_grid+1, n_comp] (include/lfsd_cpdp.h, ABI 11); n_grid >= 3."""
        if not isinstance(grid, torch.Tensor) or grid.dim() != 3:
            raise LfsdError("grid must be a [B, n_grid+1, n_comp] tensor")
        if grid.dtype not in _DT:
            raise LfsdError("grid has dtype %s: float32 or float64" % grid.dtype)
        B, N1, C = grid.shape
        self._check(grid, (B, N1, C), grid.dtype, "grid")
        if N1 < 4:
            raise LfsdError("the cubic interpolant needs n_grid >= 3 (four nodes), got n_grid = %d" % (N1 - 1))
        if out is None:
            out = torch.empty_like(grid)
        self._check(out, (B, N1, C), grid.dtype, "out")
        if out.data_ptr() == grid.data_ptr():
            raise LfsdError("grid_curvature does not run in place")
        with self._on(grid):
            rc = self.lib.lfsd_grid_curvature(_DT[grid.dtype], B, N1 - 1, C, self._p(grid), self._p(out), self._stream(grid))
        self._rc(rc, "lfsd_grid_curvature")
        return out

    def sample_grid(self, grid, horizon, times, curv=None, out=None):
        """The batched call of an interpolant (include/lfsd_cpdp.h, ABI 12): ``interp1d(time_grid, grid[b])(times)`` for every
        trajectory -- linear (CPDP.py:386) or, with ``curv`` (``grid_curvature(grid)``), scipy's cubic (CPDP.py:388-390).
        grid [B, n_grid+1, C], horizon [B], times [B, K] or [K] (shared by the batch) -> [B, K, C].  Times outside [0, horizon]
        extrapolate the end interval (the range check is the caller's: COCSys.sampleBatch); a NaN time gives a NaN row."""
        if not isinstance(grid, torch.Tensor) or grid.dim() != 3:
            raise LfsdError("grid must be a [B, n_grid+1, n_comp] tensor")
        if grid.dtype not in _DT:
            raise LfsdError("grid has dtype %s: float32 or float64" % grid.dtype)
        dt = grid.dtype
        B, N1, C = grid.shape
        self._check(grid, (B, N1, C), dt, "grid")
        self._check(horizon, (B,), dt, "horizon")
        if not isinstance(times, torch.Tensor) or times.dim() not in (1, 2) or times.shape[-1] < 1:
            raise LfsdError("times must be a [B, K] or [K] tensor with K >= 1")
        K = times.shape[-1]
        self._check(times, (B, K) if times.dim() == 2 else (K,), dt, "times")
        if N1 < 2 or (curv is not None and N1 < 4):
            raise LfsdError("n_grid = %d: the linear interpolant needs two nodes, the cubic one four" % (N1 - 1))
        self._check(curv, (B, N1, C), dt, "curv", optional=True)
        if out is None:
            out = torch.empty((B, K, C), dtype=dt, device=grid.device)
        self._check(out, (B, K, C), dt, "out")
        with self._on(grid):
            rc = self.lib.lfsd_sample_grid(_DT[dt], B, N1 - 1, C, K, 1 if times.dim() == 2 else 0, self._p(grid), self._p(curv),
                                           self._p(horizon), self._p(times), self._p(out), self._stream(grid))
        self._rc(rc, "lfsd_sample_grid")
        return out

    def waypoint_vjp(self, horizon, taus, rx, auxX_grid, ru=None, auxU_grid=None, out=None):
        """grad [B, p] = sum_k rx[:, k] . dx/dtheta(tau_k) (+ ru[:, k] . du/dtheta(tau_k)) on the linear interpolants of the
        sensitivity grids (include/lfsd_cpdp.h, ABI 12): the chain rule of a user-written loss through ``auxsys_sol``.
        horizon [B], taus [B, K], rx [B, K, n], auxX_grid [B, n_grid+1, p, n]; ru [B, K, m] and auxU_grid [B, n_grid+1, p, m]
        together or not at all.  Fixed summation order: a row's gradient is the same bits in any batch."""
        if not isinstance(auxX_grid, torch.Tensor) or auxX_grid.dim() != 4:
            raise LfsdError("auxX_grid must be a [B, n_grid+1, n_param, n_state] tensor")
        if auxX_grid.dtype not in _DT:
            raise LfsdError("auxX_grid has dtype %s: float32 or float64" % auxX_grid.dtype)
        dt = auxX_grid.dtype
        B, N1, p, n = auxX_grid.shape
        if (ru is None) != (auxU_grid is None):
            raise LfsdError("ru and auxU_grid go together")
        if not isinstance(taus, torch.Tensor) or taus.dim() != 2 or taus.shape[1] < 1:
            raise LfsdError("taus must be a [B, K] tensor with K >= 1")
        K = taus.shape[1]
        self._check(auxX_grid, (B, N1, p, n), dt, "auxX_grid")
        self._check(horizon, (B,), dt, "horizon")
        self._check(taus, (B, K), dt, "taus")
        self._check(rx, (B, K, n), dt, "rx")
        m = self.n_control
        if ru is not None:
            if not isinstance(auxU_grid, torch.Tensor) or auxU_grid.dim() != 4:
                raise LfsdError("auxU_grid must be a [B, n_grid+1, n_param, n_control] tensor")
            m = auxU_grid.shape[3]
            self._check(auxU_grid, (B, N1, p, m), dt, "auxU_grid")
            self._check(ru, (B, K, m), dt, "ru")
        if N1 < 2:
            raise LfsdError("n_grid = %d: the interpolant needs two nodes" % (N1 - 1))
        if out is None:
            out = torch.empty((B, p), dtype=dt, device=auxX_grid.device)
        self._check(out, (B, p), dt, "out")
        with self._on(auxX_grid):
            rc = self.lib.lfsd_waypoint_vjp(_DT[dt], B, N1 - 1, n, m, p, K, self._p(horizon), self._p(taus), self._p(rx), self._p(ru),
                                            self._p(auxX_grid), self._p(auxU_grid), self._p(out), self._stream(auxX_grid))
        self._rc(rc, "lfsd_waypoint_vjp")
        return out

    def aux_solve(self, horizon, auxvar, consts, state_grid, control_grid, costate_grid, taus, waypoints, iface_idx,
                  substeps=0, want_grids=False, Z_grid=None, out=None, phase_hook=None, rtol=1e-3, oc_status=None,
                  skip_status=(), interp_level=1, curvature=None, wp_weight=None, auxX_grid=None, auxU_grid=None):
        """``auxX_grid`` [B, n_grid+1, p, n] / ``auxU_grid`` [B, n_grid+1, p, m] (with ``want_grids``): the caller's buffers for the
        sensitivity grids, as ``Z_grid`` is for [P W]; allocated here otherwise.
        ``wp_weight`` [B, K] or None (include/lfsd_cpdp.h, ABI 16): a weight per waypoint, loss = sum_k w_k |r_k|^2; a zero weight
        removes the waypoint (its tau and target are not read); non-negative and finite, which the caller guarantees (nothing is
        read back here).  With weights the call is ``lfsd_aux_riccati`` then ``lfsd_aux_forward_weighted`` (there is no weighted
        ``lfsd_aux_solve``); None: the launches as ever.
        ``interp_level`` 1: the sweeps differentiate along the linear interpolant of the grids (CPDP.py:386); 2: along their cubic
        interpolant (CPDP.py:388-390; the ``*_cubic`` entry points).  ``curvature``: at level 2, the (state, control, costate)
        curvature tensors if the caller has them (``grid_curvature``); fitted here otherwise; returned as ``out["curvature"]``.
        ``phase_hook(name)``, if given, is called before/after each of the two launches
        ("riccati", "forward") so a caller can bracket them with HIP events (bench.py).
        ``oc_status`` [B] int32 (the status the OC solve wrote) + ``skip_status`` (status values, e.g. (3, 4)): rows with
        one of these statuses are not differentiated -- NaN loss / gradient, no sweep (include/lfsd_cpdp.h, ABI 8)."""
        dt = state_grid.dtype
        B, N1, n = state_grid.shape
        N = N1 - 1
        m, p, nc = self.n_control, self.n_auxvar, self.n_const
        dev = state_grid.device
        self._check(horizon, (B,), dt, "horizon")
        self._check(auxvar, (B, p), dt, "auxvar")
        self._check(state_grid, (B, N + 1, self.n_state), dt, "state_grid")
        self._check(control_grid, (B, N + 1, m), dt, "control_grid")
        self._check(costate_grid, (B, N + 1, n), dt, "costate_grid")
        per_traj = 0
        if nc:
            if consts is None:
                raise LfsdError("consts is required (n_const=%d)" % nc)
            if consts.dim() == 2:
                self._check(consts, (B, nc), dt, "consts")
                per_traj = 1
            else:
                self._check(consts, (nc,), dt, "consts")
        else:
            consts = None
        nw = 0 if taus is None else taus.shape[1]
        ni = 0 if iface_idx is None else iface_idx.shape[0]
        if nw and iface_idx is None:      # the interface function compiled into the library (COCSys.setInterface)
            ni = self.n_interface
            if ni == 0:
                raise LfsdError("no interface_idx given and the model library carries no compiled interface function")
        if nw:
            self._check(taus, (B, nw), dt, "taus")
            self._check(waypoints, (B, nw, ni), dt, "waypoints")
            self._check(iface_idx, (ni,), torch.int32, "iface_idx", optional=True)
            self._check(wp_weight, (B, nw), dt, "wp_weight", optional=True)
        elif wp_weight is not None:
            raise LfsdError("wp_weight without waypoints")
        if Z_grid is None:
            Z_grid = torch.empty((B, N + 1, n + p, n), dtype=dt, device=dev)
        if out is None:
            out = dict(loss=torch.zeros((B,), dtype=dt, device=dev), grad=torch.zeros((B, p), dtype=dt, device=dev))
        if out.get("stats") is None:
            # [B][4]: split units executed / intervals accepted above rtol, Riccati sweep | forward sweep (include/lfsd_cpdp.h)
            out["stats"] = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        self._check(out["stats"], (B, 4), torch.int32, "stats")
        skip_mask = 0
        for st in skip_status:
            if not 0 <= int(st) < 31:
                raise LfsdError("skip_status values must be OC-solve statuses (0..30)")
            skip_mask |= 1 << int(st)
        if skip_mask or oc_status is not None:      # (without a mask the status still tells the sweeps which rows to budget)
            self._check(oc_status, (B,), torch.int32, "oc_status")
        if interp_level not in (1, 2):
            raise LfsdError("interp_level must be 1 (linear) or 2 (cubic), got %r" % (interp_level,))
        curv = ()
        if interp_level == 2:
            if N < 3:
                raise LfsdError("the cubic interpolant needs n_grid >= 3 (four nodes), got n_grid = %d" % N)
            grids = (state_grid, control_grid, costate_grid)
            if curvature is None:
                curvature = tuple(self.grid_curvature(g) for g in grids)
            if len(curvature) != 3:
                raise LfsdError("curvature is the triple (state, control, costate)")
            for g, c, nm in zip(grids, curvature, ("state_curv", "control_curv", "costate_curv")):
                self._check(c, tuple(g.shape), dt, nm)
            curv = tuple(self._p(c) for c in curvature)
        elif curvature is not None:
            raise LfsdError("curvature tensors belong to interp_level=2")
        sfx = "_cubic" if interp_level == 2 else ""
        auxX = auxU = None
        if (auxX_grid is not None or auxU_grid is not None) and not want_grids:
            raise LfsdError("auxX_grid / auxU_grid buffers belong to want_grids=True")
        if want_grids:
            auxX = torch.empty((B, N + 1, p, n), dtype=dt, device=dev) if auxX_grid is None else auxX_grid
            auxU = torch.empty((B, N + 1, p, m), dtype=dt, device=dev) if auxU_grid is None else auxU_grid
            self._check(auxX, (B, N + 1, p, n), dt, "auxX_grid")
            self._check(auxU, (B, N + 1, p, m), dt, "auxU_grid")
        common = (_DT[dt], B, N, self._p(horizon), self._p(auxvar), self._p(consts), per_traj,
                  self._p(state_grid), self._p(control_grid), self._p(costate_grid)) + curv + (self._p(Z_grid),)
        tail = (nw, ni, self._p(iface_idx), self._p(taus), self._p(waypoints), self._p(out["loss"]),
                self._p(out["grad"]), self._p(auxX), self._p(auxU), int(substeps), float(rtol), self._p(out["stats"]),
                self._p(oc_status), skip_mask, self._stream(state_grid))
        fwd = "lfsd_aux_forward" + sfx
        if wp_weight is not None:      # the weighted forward sweep: wp_weight goes after waypoints
            fwd += "_weighted"
            tail = tail[:5] + (self._p(wp_weight),) + tail[5:]
            if phase_hook is None:
                phase_hook = lambda name: None
        with self._on(state_grid):
            if phase_hook is None:
                self._rc(getattr(self.lib, "lfsd_aux_solve" + sfx)(*common, *tail), "lfsd_aux_solve" + sfx)
            else:
                phase_hook("riccati")
                self._rc(getattr(self.lib, "lfsd_aux_riccati" + sfx)(*common, int(substeps), float(rtol), self._p(out["stats"]),
                                                                     self._p(oc_status), skip_mask, self._stream(state_grid)),
                         "lfsd_aux_riccati" + sfx)
                phase_hook("forward")
                self._rc(getattr(self.lib, fwd)(*common, *tail), fwd)
                phase_hook("end")
        out["Z_grid"] = Z_grid
        out["auxX_grid"], out["auxU_grid"] = auxX, auxU
        out["curvature"] = curvature if interp_level == 2 else None
        return out

    def optimizer_step(self, method, theta, grad, iter_idx, lr, mu=0.9, beta1=0.9, beta2=0.999, eps=1e-8, m=None,
                       v=None, vhat=None, proj_lo=None, row_active=None):
        dt = theta.dtype
        B, p = theta.shape
        for nm, t in (("theta", theta), ("grad", grad)):
            self._check(t, (B, p), dt, nm)
        for nm, t in (("m", m), ("v", v), ("vhat", vhat)):
            self._check(t, (B, p), dt, nm, optional=True)
        self._check(proj_lo, (p,), dt, "proj_lo", optional=True)
        self._check(row_active, (B,), torch.int32, "row_active", optional=True)
        with self._on(theta):
            rc = self.lib.lfsd_optimizer_step(_DT[dt], OPT_METHODS[method] if isinstance(method, str) else int(method),
                                              B, p, int(iter_idx), float(lr), float(mu), float(beta1), float(beta2),
                                              float(eps), self._p(theta), self._p(grad), self._p(m), self._p(v),
                                              self._p(vhat), self._p(proj_lo), self._p(row_active),
                                              self._stream(theta))
        self._rc(rc, "lfsd_optimizer_step")

    def lookahead(self, theta, v, mu, out=None):
        if out is None:
            out = torch.empty_like(theta)
        with self._on(theta):
            rc = self.lib.lfsd_lookahead(_DT[theta.dtype], theta.numel(), float(mu), self._p(theta), self._p(v),
                                         self._p(out), self._stream(theta))
        self._rc(rc, "lfsd_lookahead")
        return out

    # ---- ABI 13: per-row update rules and device traces -------------------------------------------------------------------
    def _rows_args(self, method, hyper, theta):
        if not isinstance(theta, torch.Tensor) or theta.dim() != 2 or theta.dtype not in _DT:
            raise LfsdError("theta must be a [B, n_param] float32 / float64 tensor")
        B, p = theta.shape
        self._check(theta, (B, p), theta.dtype, "theta")
        self._check(method, (B,), torch.int32, "method")
        self._check(hyper, (B, 5), theta.dtype, "hyper")
        return B, p, theta.dtype

    def optimizer_step_rows(self, method, hyper, theta, grad, iter_idx, m, v, vhat, proj_lo=None, row_active=None):
        """``optimizer_step`` with the rule and the hyper-parameters per row (include/lfsd_cpdp.h, ABI 13): method [B] int32
        (runtime.OPT_METHODS codes), hyper [B, 5] = lr, mu, beta1, beta2, eps in theta's dtype.  Bit for bit what ``optimizer_step``
        gives each row with its own values; m, v, vhat are all required (the batch may mix rules)."""
        B, p, dt = self._rows_args(method, hyper, theta)
        for nm, t in (("grad", grad), ("m", m), ("v", v), ("vhat", vhat)):
            self._check(t, (B, p), dt, nm)
        self._check(proj_lo, (p,), dt, "proj_lo", optional=True)
        self._check(row_active, (B,), torch.int32, "row_active", optional=True)
        with self._on(theta):
            rc = self.lib.lfsd_optimizer_step_rows(_DT[dt], B, p, int(iter_idx), self._p(method), self._p(hyper), self._p(theta),
                                                   self._p(grad), self._p(m), self._p(v), self._p(vhat), self._p(proj_lo),
                                                   self._p(row_active), self._stream(theta))
        self._rc(rc, "lfsd_optimizer_step_rows")

    def lookahead_rows(self, method, hyper, theta, m, out=None):
        """The evaluation point of a mixed batch: theta + mu_b * m for Nesterov rows, a bit copy of theta for every other row."""
        B, p, dt = self._rows_args(method, hyper, theta)
        self._check(m, (B, p), dt, "m")
        if out is None:
            out = torch.empty_like(theta)
        self._check(out, (B, p), dt, "out")
        with self._on(theta):
            rc = self.lib.lfsd_lookahead_rows(_DT[dt], B, p, self._p(method), self._p(hyper), self._p(theta), self._p(m),
                                              self._p(out), self._stream(theta))
        self._rc(rc, "lfsd_lookahead_rows")
        return out

    def trace_append(self, iter_idx, loss, grad, theta, loss_trace=None, gnorm_trace=None, theta_trace=None, row_active=None):
        """File loss[b], ||grad[b]||_2 and theta[b] of every active row under iteration ``iter_idx`` (include/lfsd_cpdp.h, ABI 13):
        loss_trace / gnorm_trace [B, capacity] at [:, iter_idx], theta_trace [B, capacity+1, p] at [:, iter_idx+1].  Any of the
        three may be None, not all.  Nothing is read back."""
        if not isinstance(theta, torch.Tensor) or theta.dim() != 2 or theta.dtype not in _DT:
            raise LfsdError("theta must be a [B, n_param] float32 / float64 tensor")
        B, p = theta.shape
        dt = theta.dtype
        self._check(theta, (B, p), dt, "theta")
        self._check(grad, (B, p), dt, "grad")
        self._check(loss, (B,), dt, "loss")
        given = [t for t in (loss_trace, gnorm_trace) if t is not None]
        if theta_trace is not None:
            if not isinstance(theta_trace, torch.Tensor) or theta_trace.dim() != 3:
                raise LfsdError("theta_trace must be a [B, capacity+1, n_param] tensor")
            cap = theta_trace.shape[1] - 1
        elif given:
            if not isinstance(given[0], torch.Tensor) or given[0].dim() != 2:
                raise LfsdError("loss_trace / gnorm_trace must be [B, capacity] tensors")
            cap = given[0].shape[1]
        else:
            raise LfsdError("trace_append needs at least one of loss_trace, gnorm_trace, theta_trace")
        self._check(loss_trace, (B, cap), dt, "loss_trace", optional=True)
        self._check(gnorm_trace, (B, cap), dt, "gnorm_trace", optional=True)
        self._check(theta_trace, (B, cap + 1, p), dt, "theta_trace", optional=True)
        self._check(row_active, (B,), torch.int32, "row_active", optional=True)
        if not 0 <= int(iter_idx) < cap:
            raise LfsdError("iteration %d does not fit a trace of capacity %d" % (int(iter_idx), cap))
        with self._on(theta):
            rc = self.lib.lfsd_trace_append(_DT[dt], B, p, int(iter_idx), cap, self._p(loss), self._p(grad), self._p(theta),
                                            self._p(row_active), self._p(loss_trace), self._p(gnorm_trace), self._p(theta_trace),
                                            self._stream(theta))
        self._rc(rc, "lfsd_trace_append")

    # ---- ABI 14: Gauss-Newton matrix of the waypoint loss, Levenberg-Marquardt step --------------------------------------------
    def normal_matrix(self, horizon, taus, auxX_grid, iface_idx, out=None, wp_weight=None):
        """``wp_weight`` [B, K] or None (ABI 16): H = sum_k w_k J_k^T J_k through ``lfsd_normal_matrix_weighted``; a zero weight removes
        the waypoint; None: ``lfsd_normal_matrix`` as ever.
        H [B, p, p] = J^T J of the waypoint residuals (include/lfsd_cpdp.h, ABI 14): J is the linear interpolant of ``auxX_grid``
        [B, n_grid+1, p, n] at ``taus`` [B, K], restricted to the state components ``iface_idx`` [n_iface] int32.  horizon [B].
        Exactly symmetric; fixed summation order: a row's H is the same bits in any batch.  An entry of ``iface_idx`` outside
        [0, n) is found on the device (nothing is read back here): the call then writes nothing.  Small eigenvalues of H are
        directions of theta the waypoints do not pin down."""
        if not isinstance(auxX_grid, torch.Tensor) or auxX_grid.dim() != 4:
            raise LfsdError("auxX_grid must be a [B, n_grid+1, n_param, n_state] tensor")
        if auxX_grid.dtype not in _DT:
            raise LfsdError("auxX_grid has dtype %s: float32 or float64" % auxX_grid.dtype)
        dt = auxX_grid.dtype
        B, N1, p, n = auxX_grid.shape
        if not isinstance(taus, torch.Tensor) or taus.dim() != 2 or taus.shape[1] < 1:
            raise LfsdError("taus must be a [B, K] tensor with K >= 1")
        if not isinstance(iface_idx, torch.Tensor) or iface_idx.dim() != 1 or iface_idx.shape[0] < 1:
            raise LfsdError("iface_idx must be an int32 tensor of at least one state component")
        K, ni = taus.shape[1], iface_idx.shape[0]
        self._check(auxX_grid, (B, N1, p, n), dt, "auxX_grid")
        self._check(horizon, (B,), dt, "horizon")
        self._check(taus, (B, K), dt, "taus")
        self._check(iface_idx, (ni,), torch.int32, "iface_idx")
        if N1 < 2:
            raise LfsdError("n_grid = %d: the interpolant needs two nodes" % (N1 - 1))
        if out is None:
            out = torch.empty((B, p, p), dtype=dt, device=auxX_grid.device)
        self._check(out, (B, p, p), dt, "out")
        self._check(wp_weight, (B, K), dt, "wp_weight", optional=True)
        with self._on(auxX_grid):
            if wp_weight is None:
                rc = self.lib.lfsd_normal_matrix(_DT[dt], B, N1 - 1, n, p, K, ni, self._p(iface_idx), self._p(horizon), self._p(taus),
                                                 self._p(auxX_grid), self._p(out), self._stream(auxX_grid))
            else:
                rc = self.lib.lfsd_normal_matrix_weighted(_DT[dt], B, N1 - 1, n, p, K, ni, self._p(iface_idx), self._p(horizon),
                                                          self._p(taus), self._p(wp_weight), self._p(auxX_grid), self._p(out),
                                                          self._stream(auxX_grid))
        self._rc(rc, "lfsd_normal_matrix" if wp_weight is None else "lfsd_normal_matrix_weighted")
        return out

    def lm_step(self, theta, loss_acc, grad_acc, H_acc, lam, theta_trial, loss_t, grad_t, H_t, lambda_down=1.0 / 3.0, lambda_up=2.0,
                lambda_min=1e-8, lambda_max=1e8, proj_lo=None, row_active=None, accepted=None):
        """One Levenberg-Marquardt update of every row, in place (include/lfsd_cpdp.h, ABI 14): accept or reject the evaluation
        (loss_t [B], grad_t [B, p], H_t [B, p, p]) of ``theta_trial``, adapt ``lam`` [B], and leave in ``theta_trial`` the next
        point to evaluate.  theta / grad_acc [B, p], loss_acc [B] (+inf: nothing accepted yet), H_acc [B, p, p]; p <= 16.
        ``accepted`` [B] int32 or None.  Nothing is read back."""
        if not isinstance(theta, torch.Tensor) or theta.dim() != 2 or theta.dtype not in _DT:
            raise LfsdError("theta must be a [B, n_param] float32 / float64 tensor")
        B, p = theta.shape
        dt = theta.dtype
        if p > 16:
            raise LfsdError("lm_step factors a p x p matrix per lane: n_param = %d > 16" % p)
        for nm, t in (("theta", theta), ("grad_acc", grad_acc), ("theta_trial", theta_trial), ("grad_t", grad_t)):
            self._check(t, (B, p), dt, nm)
        for nm, t in (("loss_acc", loss_acc), ("lambda", lam), ("loss_t", loss_t)):
            self._check(t, (B,), dt, nm)
        for nm, t in (("H_acc", H_acc), ("H_t", H_t)):
            self._check(t, (B, p, p), dt, nm)
        self._check(proj_lo, (p,), dt, "proj_lo", optional=True)
        self._check(row_active, (B,), torch.int32, "row_active", optional=True)
        self._check(accepted, (B,), torch.int32, "accepted", optional=True)
        with self._on(theta):
            rc = self.lib.lfsd_lm_step(_DT[dt], B, p, float(lambda_down), float(lambda_up), float(lambda_min), float(lambda_max),
                                       self._p(theta), self._p(loss_acc), self._p(grad_acc), self._p(H_acc), self._p(lam),
                                       self._p(theta_trial), self._p(loss_t), self._p(grad_t), self._p(H_t), self._p(proj_lo),
                                       self._p(row_active), self._p(accepted), self._stream(theta))
        self._rc(rc, "lfsd_lm_step")

    # ---- ABI 15: several demonstrations per seed -- the per-group sums -------------------------------------------------------------
    def group_reduce(self, loss, grad, group_size, H=None, row_ok=None, out=None):
        """Sums of loss [B], grad [B, p] and (optionally) H [B, p, p] over the ``group_size`` consecutive rows of every group
        (include/lfsd_cpdp.h, ABI 15): row ``g * group_size + d`` is demonstration d of group g.  ``row_ok`` [B] int32 or None: rows
        with 0 are left out (their values may be NaN).  Returns ``(loss_g [G], grad_g [G, p], H_g [G, p, p] or None, n_ok [G] int32)``;
        ``out``: such a tuple to write into.  Fixed summation order (0, then the rows ascending): a group's sums are the same bits in
        any batch.  Nothing is read back."""
        if not isinstance(grad, torch.Tensor) or grad.dim() != 2 or grad.dtype not in _DT:
            raise LfsdError("grad must be a [B, n_param] float32 / float64 tensor")
        B, p = grad.shape
        dt = grad.dtype
        if isinstance(group_size, bool) or int(group_size) != group_size or int(group_size) <= 0:
            raise LfsdError("group_size must be a positive integer (got %r)" % (group_size,))
        D = int(group_size)
        if B < 1 or p < 1 or B % D != 0:
            raise LfsdError("a batch of %d rows is not a whole number of groups of %d" % (B, D))
        G = B // D
        self._check(grad, (B, p), dt, "grad")
        self._check(loss, (B,), dt, "loss")
        self._check(H, (B, p, p), dt, "H", optional=True)
        self._check(row_ok, (B,), torch.int32, "row_ok", optional=True)
        if out is None:
            new = lambda *shape: torch.empty(shape, dtype=dt, device=grad.device)
            out = (new(G), new(G, p), None if H is None else new(G, p, p), torch.empty(G, dtype=torch.int32, device=grad.device))
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise LfsdError("out is a tuple (loss_g [G], grad_g [G, p], H_g [G, p, p] or None, n_ok [G])")
        loss_g, grad_g, H_g, n_ok = out
        if (H is None) != (H_g is None):
            raise LfsdError("H and out's H_g are given together or not at all")
        self._check(loss_g, (G,), dt, "loss_g")
        self._check(grad_g, (G, p), dt, "grad_g")
        self._check(H_g, (G, p, p), dt, "H_g", optional=True)
        self._check(n_ok, (G,), torch.int32, "n_ok")
        with self._on(grad):
            rc = self.lib.lfsd_group_reduce(_DT[dt], G, D, p, self._p(loss), self._p(grad), self._p(H), self._p(row_ok),
                                            self._p(loss_g), self._p(grad_g), self._p(H_g), self._p(n_ok), self._stream(grad))
        self._rc(rc, "lfsd_group_reduce")
        return loss_g, grad_g, H_g, n_ok

    # ---- ABI 17: learnable waypoint times ---------------------------------------------------------------------------------------------
    def waypoint_time_grad(self, state_grid, horizon, taus, waypoints, iface_idx, curv=None, consts=None, wp_weight=None,
                           tau_ref=None, tau_prior=0.0, out=None):
        """dtau [B, K] = w_k r^T dy/dx xdot(tau_k) + tau_prior (tau_k - tau_ref_k): half the derivative of the fused waypoint loss
        in the waypoint times (include/lfsd_cpdp.h, ABI 17).  state_grid [B, n_grid+1, n], horizon [B], taus [B, K], waypoints
        [B, K, n_iface]; ``iface_idx`` [n_iface] int32, or None for the interface compiled into the library (then ``consts`` as
        aux_solve takes them); ``curv`` = ``grid_curvature(state_grid)`` for the cubic interpolant; ``wp_weight`` / ``tau_ref``
        [B, K] or None.  A waypoint of weight 0 gets +0 and is never read.  Nothing is read back."""
        if not isinstance(state_grid, torch.Tensor) or state_grid.dim() != 3 or state_grid.dtype not in _DT:
            raise LfsdError("state_grid must be a [B, n_grid+1, n_state] float32 / float64 tensor")
        dt = state_grid.dtype
        B, N1, n = state_grid.shape
        if n != self.n_state:
            raise LfsdError("state_grid has %d state components, the model %d" % (n, self.n_state))
        if N1 < 2 or (curv is not None and N1 < 4):
            raise LfsdError("n_grid = %d: the linear interpolant needs two nodes, the cubic one four" % (N1 - 1))
        if not isinstance(taus, torch.Tensor) or taus.dim() != 2 or taus.shape[1] < 1:
            raise LfsdError("taus must be a [B, K] tensor with K >= 1")
        K = taus.shape[1]
        per_traj = 0
        if iface_idx is None:
            ni = self.n_interface
            if ni == 0:
                raise LfsdError("iface_idx=None selects the interface compiled into the library: this one has none")
            if self.n_const:
                if not isinstance(consts, torch.Tensor):
                    raise LfsdError("consts is required by the compiled interface (n_const=%d)" % self.n_const)
                per_traj = 1 if consts.dim() == 2 else 0
                self._check(consts, (B, self.n_const) if per_traj else (self.n_const,), dt, "consts")
            else:
                consts = None
        else:
            if not isinstance(iface_idx, torch.Tensor) or iface_idx.dim() != 1 or iface_idx.shape[0] < 1:
                raise LfsdError("iface_idx must be an int32 tensor of at least one state component")
            ni = iface_idx.shape[0]
            self._check(iface_idx, (ni,), torch.int32, "iface_idx")
            consts = None
        self._check(state_grid, (B, N1, n), dt, "state_grid")
        self._check(curv, (B, N1, n), dt, "curv", optional=True)
        self._check(horizon, (B,), dt, "horizon")
        self._check(taus, (B, K), dt, "taus")
        self._check(waypoints, (B, K, ni), dt, "waypoints")
        self._check(wp_weight, (B, K), dt, "wp_weight", optional=True)
        self._check(tau_ref, (B, K), dt, "tau_ref", optional=True)
        if out is None:
            out = torch.empty((B, K), dtype=dt, device=state_grid.device)
        self._check(out, (B, K), dt, "out")
        with self._on(state_grid):
            rc = self.lib.lfsd_waypoint_time_grad(_DT[dt], B, N1 - 1, K, ni, self._p(state_grid), self._p(curv), self._p(horizon),
                                                  self._p(consts), per_traj, self._p(taus), self._p(waypoints), self._p(iface_idx),
                                                  self._p(wp_weight), self._p(tau_ref), float(tau_prior), self._p(out),
                                                  self._stream(state_grid))
        self._rc(rc, "lfsd_waypoint_time_grad")
        return out

    def tau_project(self, tau_ref, tau_io, horizon, max_shift, wp_weight=None, tau_lo=None, tau_hi=None, row_active=None):
        """In place: ``tau_io`` [B, K] clamped to within ``max_shift`` (0 < c < 0.5) of the gap to the neighbours in the ordered
        times ``tau_ref`` [B, K] (0 and horizon [B] at the ends), and to ``tau_lo`` / ``tau_hi`` [B, K] first (include/lfsd_cpdp.h,
        ABI 17): the order of a row cannot invert.  Waypoints of weight 0 and rows with ``row_active`` == 0 keep their words; a
        non-finite proposal keeps the reference time.  Returns ``tau_io``.  Nothing is read back."""
        if not isinstance(tau_io, torch.Tensor) or tau_io.dim() != 2 or tau_io.dtype not in _DT or tau_io.shape[1] < 1:
            raise LfsdError("tau_io must be a [B, K] float32 / float64 tensor with K >= 1")
        dt = tau_io.dtype
        B, K = tau_io.shape
        self._check(tau_io, (B, K), dt, "tau_io")
        self._check(tau_ref, (B, K), dt, "tau_ref")
        self._check(horizon, (B,), dt, "horizon")
        self._check(wp_weight, (B, K), dt, "wp_weight", optional=True)
        self._check(tau_lo, (B, K), dt, "tau_lo", optional=True)
        self._check(tau_hi, (B, K), dt, "tau_hi", optional=True)
        self._check(row_active, (B,), torch.int32, "row_active", optional=True)
        if tau_ref.data_ptr() == tau_io.data_ptr():
            raise LfsdError("tau_project clamps tau_io against tau_ref: they are two arrays")
        with self._on(tau_io):
            rc = self.lib.lfsd_tau_project(_DT[dt], B, K, self._p(tau_ref), self._p(tau_io), self._p(horizon), self._p(wp_weight),
                                           self._p(tau_lo), self._p(tau_hi), float(max_shift), self._p(row_active),
                                           self._stream(tau_io))
        self._rc(rc, "lfsd_tau_project")
        return tau_io

    # ---- ABI 18: Levenberg-Marquardt over parameters and waypoint times jointly ------------------------------------------------------
    def time_normal_blocks(self, state_grid, horizon, taus, auxX_grid, iface_idx, curv=None, wp_weight=None, out=None):
        """(C [B, K, p], d [B, K]): the coupling c_k = w_k J_k^T t_k and the time block d_k = w_k t_k^T t_k of the Gauss-Newton matrix
        in (theta, tau) (include/lfsd_cpdp.h, ABI 18).  J_k is the linear interpolant of ``auxX_grid`` [B, n_grid+1, p, n] at ``taus``
        [B, K] on ``iface_idx`` [n_iface] int32, t_k the interface rows of the slope of ``state_grid`` [B, n_grid+1, n] there (with
        ``curv`` = ``grid_curvature(state_grid)`` along the cubic interpolant).  ``wp_weight`` [B, K] or None; a waypoint of weight 0
        gets +0 and is never read.  ``out``: such a pair to write into.  Nothing is read back."""
        if not isinstance(auxX_grid, torch.Tensor) or auxX_grid.dim() != 4 or auxX_grid.dtype not in _DT:
            raise LfsdError("auxX_grid must be a [B, n_grid+1, n_param, n_state] float32 / float64 tensor")
        dt = auxX_grid.dtype
        B, N1, p, n = auxX_grid.shape
        if not isinstance(taus, torch.Tensor) or taus.dim() != 2 or taus.shape[1] < 1:
            raise LfsdError("taus must be a [B, K] tensor with K >= 1")
        if not isinstance(iface_idx, torch.Tensor) or iface_idx.dim() != 1 or iface_idx.shape[0] < 1:
            raise LfsdError("iface_idx must be an int32 tensor of at least one state component")
        K, ni = taus.shape[1], iface_idx.shape[0]
        if N1 < 2 or (curv is not None and N1 < 4):
            raise LfsdError("n_grid = %d: the linear interpolant needs two nodes, the cubic one four" % (N1 - 1))
        self._check(auxX_grid, (B, N1, p, n), dt, "auxX_grid")
        self._check(state_grid, (B, N1, n), dt, "state_grid")
        self._check(curv, (B, N1, n), dt, "curv", optional=True)
        self._check(horizon, (B,), dt, "horizon")
        self._check(taus, (B, K), dt, "taus")
        self._check(wp_weight, (B, K), dt, "wp_weight", optional=True)
        self._check(iface_idx, (ni,), torch.int32, "iface_idx")
        if out is None:
            out = (torch.empty((B, K, p), dtype=dt, device=auxX_grid.device), torch.empty((B, K), dtype=dt, device=auxX_grid.device))
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise LfsdError("out is a pair (C [B, K, p], d [B, K])")
        C, d = out
        self._check(C, (B, K, p), dt, "C")
        self._check(d, (B, K), dt, "d")
        with self._on(auxX_grid):
            rc = self.lib.lfsd_time_normal_blocks(_DT[dt], B, N1 - 1, n, p, K, ni, self._p(iface_idx), self._p(horizon), self._p(taus),
                                                  self._p(wp_weight), self._p(state_grid), self._p(curv), self._p(auxX_grid),
                                                  self._p(C), self._p(d), self._stream(auxX_grid))
        self._rc(rc, "lfsd_time_normal_blocks")
        return C, d

    def lm_step_times(self, theta, loss_acc, grad_acc, H_acc, lam, theta_trial, tau, tau_trial, gtau_acc, C_acc, d_acc, ok_acc,
                      loss_t, grad_t, H_t, gtau_t, C_t, d_t, group_size=1, lambda_down=1.0 / 3.0, lambda_up=2.0, lambda_min=1e-8,
                      lambda_max=1e8, row_ok=None, wp_weight=None, proj_lo=None, group_active=None, accepted=None):
        """One Levenberg-Marquardt update over (theta, tau) of every group, in place (include/lfsd_cpdp.h, ABI 18): ``lm_step`` with
        the times of the group's ``group_size`` rows as unknowns, eliminated per waypoint.  Per group: theta / grad_acc / theta_trial
        / grad_t [G, p], loss_acc / lam / loss_t [G], H_acc / H_t [G, p, p].  Per row (B = G * group_size): tau / tau_trial / gtau_acc /
        d_acc / gtau_t / d_t [B, K], C_acc / C_t [B, K, p], ok_acc [B] int32.  ``row_ok`` [B] int32, ``wp_weight`` [B, K],
        ``group_active`` / ``accepted`` [G] int32, or None.  ``tau_trial`` comes out unprojected: ``tau_project(tau, tau_trial, ...)``
        follows.  Nothing is read back."""
        if not isinstance(theta, torch.Tensor) or theta.dim() != 2 or theta.dtype not in _DT:
            raise LfsdError("theta must be a [G, n_param] float32 / float64 tensor")
        G, p = theta.shape
        dt = theta.dtype
        if p > 16:
            raise LfsdError("lm_step_times factors a p x p matrix per lane: n_param = %d > 16" % p)
        if isinstance(group_size, bool) or int(group_size) != group_size or int(group_size) <= 0:
            raise LfsdError("group_size must be a positive integer (got %r)" % (group_size,))
        D = int(group_size)
        if not isinstance(tau, torch.Tensor) or tau.dim() != 2 or tau.shape[0] != G * D or tau.shape[1] < 1:
            raise LfsdError("tau must be a [G * group_size, K] tensor with K >= 1 (G = %d, group_size = %d)" % (G, D))
        B, K = tau.shape
        for nm, t in (("theta", theta), ("grad_acc", grad_acc), ("theta_trial", theta_trial), ("grad_t", grad_t)):
            self._check(t, (G, p), dt, nm)
        for nm, t in (("loss_acc", loss_acc), ("lambda", lam), ("loss_t", loss_t)):
            self._check(t, (G,), dt, nm)
        for nm, t in (("H_acc", H_acc), ("H_t", H_t)):
            self._check(t, (G, p, p), dt, nm)
        for nm, t in (("tau", tau), ("tau_trial", tau_trial), ("gtau_acc", gtau_acc), ("d_acc", d_acc), ("gtau_t", gtau_t), ("d_t", d_t)):
            self._check(t, (B, K), dt, nm)
        for nm, t in (("C_acc", C_acc), ("C_t", C_t)):
            self._check(t, (B, K, p), dt, nm)
        self._check(ok_acc, (B,), torch.int32, "ok_acc")
        self._check(row_ok, (B,), torch.int32, "row_ok", optional=True)
        self._check(wp_weight, (B, K), dt, "wp_weight", optional=True)
        self._check(proj_lo, (p,), dt, "proj_lo", optional=True)
        self._check(group_active, (G,), torch.int32, "group_active", optional=True)
        self._check(accepted, (G,), torch.int32, "accepted", optional=True)
        P = self._p
        with self._on(theta):
            rc = self.lib.lfsd_lm_step_times(_DT[dt], G, D, p, K, float(lambda_down), float(lambda_up), float(lambda_min), float(lambda_max),
                                             P(theta), P(loss_acc), P(grad_acc), P(H_acc), P(lam), P(theta_trial), P(tau), P(tau_trial),
                                             P(gtau_acc), P(C_acc), P(d_acc), P(ok_acc), P(loss_t), P(grad_t), P(H_t), P(gtau_t), P(C_t),
                                             P(d_t), P(row_ok), P(wp_weight), P(proj_lo), P(group_active), P(accepted), self._stream(theta))
        self._rc(rc, "lfsd_lm_step_times")

    def stop_compact(self, loss, grad, loss_tol, grad_tol, iter_idx, rows_out, pos_out, n_out, active, stop_iter, rows_in=None,
                     eligible=None):
        """The reference loop's stop test per row (lib/QuadAlgorithm.py:242) + stable compaction of the survivors, one launch
        (include/lfsd_cpdp.h, ABI 10).  loss [R], grad [R, p]; rows_in / eligible [R] int32 or None; rows_out / pos_out [>= R],
        n_out [1], active / stop_iter [full batch] int32.  Nothing is read back here."""
        dt = loss.dtype
        R, p = grad.shape
        self._check(loss, (R,), dt, "loss")
        self._check(grad, (R, p), dt, "grad")
        self._check(rows_in, (R,), torch.int32, "rows_in", optional=True)
        self._check(eligible, (R,), torch.int32, "eligible", optional=True)
        for nm, t in (("rows_out", rows_out), ("pos_out", pos_out)):
            self._check(t, t.shape if isinstance(t, torch.Tensor) else None, torch.int32, nm)
            if t.dim() != 1 or t.shape[0] < R:
                raise LfsdError("%s needs room for %d rows" % (nm, R))
        self._check(n_out, (1,), torch.int32, "n_out")
        if not isinstance(active, torch.Tensor) or not isinstance(stop_iter, torch.Tensor) or active.shape != stop_iter.shape:
            raise LfsdError("active and stop_iter are full-batch int32 tensors of one shape")
        self._check(active, active.shape, torch.int32, "active")
        self._check(stop_iter, active.shape, torch.int32, "stop_iter")
        if active.dim() != 1 or (rows_in is None and active.shape[0] < R):
            raise LfsdError("active / stop_iter are indexed by original row id: [B] with B >= the number of rows")
        with self._on(loss):
            rc = self.lib.lfsd_stop_compact(_DT[dt], R, p, self._p(loss), self._p(grad), self._p(rows_in), self._p(eligible),
                                            float(loss_tol), float(grad_tol), int(iter_idx), self._p(rows_out), self._p(pos_out),
                                            self._p(n_out), self._p(active), self._p(stop_iter), self._stream(loss))
        self._rc(rc, "lfsd_stop_compact")

    def _copy_rows(self, scatter, index, src, dst, n_rows):
        name = "lfsd_scatter_rows" if scatter else "lfsd_gather_rows"
        fn = getattr(self.lib, name)
        for nm, t in (("src", src), ("dst", dst)):
            self._check(t, t.shape if isinstance(t, torch.Tensor) else None, src.dtype if isinstance(src, torch.Tensor) else None, nm)
        self._check(index, index.shape if isinstance(index, torch.Tensor) else None, torch.int32, "index")
        if src.dim() < 1 or dst.dim() != src.dim() or tuple(src.shape[1:]) != tuple(dst.shape[1:]):
            raise LfsdError("%s: src %s and dst %s are rows of different shapes" % (name, tuple(src.shape), tuple(dst.shape)))
        n_rows = int(n_rows)
        dense, sparse = (src, dst) if scatter else (dst, src)
        if index.dim() != 1 or not 0 < n_rows <= min(index.shape[0], dense.shape[0]) or sparse.shape[0] < 1:
            raise LfsdError("%s: %d rows do not fit index %s / the dense side %s" % (name, n_rows, tuple(index.shape), tuple(dense.shape)))
        row_bytes = src.element_size() * (src[0].numel() if src.dim() > 1 else 1)
        with self._on(src):
            rc = fn(n_rows, row_bytes, self._p(index), self._p(src), self._p(dst), self._stream(src))
        self._rc(rc, name)
        return dst

    def gather_rows(self, index, src, dst, n_rows):
        """dst[i] = src[index[i]] for i < n_rows (bit copy of whole rows, any dtype; include/lfsd_cpdp.h, ABI 10).  The caller
        vouches for the entries of `index` (a device array: they are not read back) lying inside src."""
        return self._copy_rows(False, index, src, dst, n_rows)

    def scatter_rows(self, index, src, dst, n_rows):
        """dst[index[i]] = src[i] for i < n_rows (distinct entries of `index`, inside dst)."""
        return self._copy_rows(True, index, src, dst, n_rows)
