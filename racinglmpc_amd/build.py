"""Build liblmpc_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "csrc", "lmpc_capi.hip")
KDEPS = [os.path.join(_HERE, "csrc", f) for f in ("lmpc_kernels.hip.h", "lmpc_solve_common.hip.h", "lmpc_solve_mw.hip.h", "lmpc_solve_cd.hip.h", "lmpc_solve_rt.hip.h", "lmpc_variant.hip.h", "lmpc_merge.h")] + [os.path.join(os.path.dirname(_HERE), "include", "lmpc_hip.h")]
DEPS = [SRC, os.path.join(_HERE, "csrc", "lmpc_comm.hip.h"), os.path.join(_HERE, "csrc", "lmpc_noise.hip.h"), os.path.join(_HERE, "csrc", "lmpc_track.hip.h"), os.path.join(_HERE, "csrc", "lmpc_commit.hip.h"), os.path.join(_HERE, "csrc", "lmpc_metrics.hip.h"), os.path.join(_HERE, "csrc", "lmpc_trace.hip.h"), os.path.join(_HERE, "csrc", "lmpc_live.hip.h"), os.path.join(_HERE, "csrc", "lmpc_relaunch.hip.h"),os.path.join(_HERE, "csrc", "lmpc_arrays.h"), os.path.join(_HERE, "csrc", "lmpc_rows.h"), os.path.join(_HERE, "csrc", "lmpc_pick.h"), os.path.join(_HERE, "csrc", "lmpc_retain.hip.h"), os.path.join(_HERE, "csrc", "lmpc_retain.h")] + KDEPS
VSRC = os.path.join(_HERE, "csrc", "lmpc_variant.hip")
# (N, numSS_points) pairs compiled into liblmpc_hip.so itself (lmpc_capi.hip: builtin_variant) and the extra ones build() prepares as
# shared objects of their own, in parallel; anything else is built the first time a Context asks for it
BUILTIN = {(n, s) for n in (8, 12, 14, 20, 40) for s in (0, 48)}
# (first the corners of the supported range, tests/envelope_cases.py: the longest compiles, started first)
EXTRA_VARIANTS = [(64, 48), (63, 48), (32, 384), (12, 384), (64, 384), (40, 384), (64, 0), (64, 192), (12, 59), (7, 48), (2, 48), (2, 0),
                  (10, 48), (16, 48), (24, 48), (30, 48), (12, 24), (12, 36), (16, 36), (10, 0), (16, 0), (12, 60), (12, 72), (12, 96), (14, 160), (12, 360)]
OUT = os.path.join(_HERE, "liblmpc_hip.so")


# Code-generation options tried in turn until the ISA check (isa_check.py: live-range copies placed ahead of a flow block's EXEC restore -- a compiler fault that
# turns loop-invariant register arrays into garbage in some lanes) finds nothing.  All are semantically neutral; the first is the plain build.
# Machine LICM is OFF for the library (not for the variant objects): the isa_check fence first picked it as the option that clears a flagged N = 40 retry kernel
# (round 5), and the whole library measured no slower with it -- the regression kernel 13-22 % FASTER at batch 4096 (0.155 -> 0.134 ms; 2.48 -> 1.93 ms with 30 laps in use:
# less hoisting, fewer live registers), headline and sweep within +-1 % (profiles/r5zz_bench.json).  So it is a base option now, not an accident of the fence.
LIB_MLLVM = ["-mllvm", "-amdgpu-mfma-vgpr-form", "-mllvm", "-disable-machine-licm"]
SALTS = [[], ["-mllvm", "-disable-postra-machine-licm"], ["-mllvm", "-amdgpu-use-amdgpu-trackers=1"], ["-mllvm", "-amdgpu-disable-loop-alignment"]]
VARIANT_SALTS = [[], ["-mllvm", "-disable-postra-machine-licm"], ["-mllvm", "-disable-machine-licm"], ["-mllvm", "-amdgpu-use-amdgpu-trackers=1"], ["-mllvm", "-amdgpu-disable-loop-alignment"],
                 # (N = 40 with 384 safe-set points, a variant without multi-wave kernels: each single option leaves the one-wave retry kernel flagged, the third and fourth together clear it)
                 ["-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-use-amdgpu-trackers=1"]]


def compile_checked(cmd, out, verbose=False, salts=None):
    """Run `cmd` (a hipcc command line without -o), check the ISA of the result, retry with the next salt while the check reports a block; the accepted
    library replaces `out` atomically and `out`.isa.json records what was needed.  Raises if no salt gives a clean build."""
    import json
    from . import isa_check
    tmp = out + ".tmp%d" % os.getpid()
    log = []
    for salt in (SALTS if salts is None else salts):
        subprocess.check_call(cmd + salt + ["-o", tmp])
        try:
            hits, images = isa_check.check_report(tmp)      # raises when nothing could be parsed: an unread library is not a clean one
        except Exception:
            os.remove(tmp)
            raise
        log.append({"options": salt, "blocks": sorted({"%s %s" % (f, l) for f, l, _, _ in hits})})
        if not hits:
            os.replace(tmp, out)
            with open(out + ".isa.json", "w") as f:
                json.dump({"accepted_with": salt, "attempts": log, "parsed": images}, f)
            if verbose or salt:
                print("isa_check: %s accepted with options %s (%d attempt(s))" % (os.path.basename(out), salt or "none", len(log)))
            return out
    os.remove(tmp)
    raise RuntimeError("isa_check: every build of %s places live-range copies ahead of an EXEC restore: %s" % (os.path.basename(out), log))


def _current():
    return os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in DEPS)


ASAN_FLAGS = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address", "-fno-gpu-sanitize", "-shared-libsan"]      # host code under AddressSanitizer, device code as it is
ASAN_RUNTIME = "/opt/rocm/lib/llvm/lib/clang/22/lib/linux/libclang_rt.asan-x86_64.so"                     # LD_PRELOAD for python (tools/asan_run.sh)


def build_flavour(suffix, defines, verbose=False, extra=(), vgpr_form=True):
    """Developer builds next to the product library (e.g. the -DLMPC_TIMING flavour of tools/phase_timing.py): liblmpc_hip_<suffix>.so.
    vgpr_form=False drops `-mllvm -amdgpu-mfma-vgpr-form` (an A / B of the compiler option itself, tools/n40_experiments.py)."""
    out = os.path.join(_HERE, "liblmpc_hip_%s.so" % suffix)
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17"] + (LIB_MLLVM if vgpr_form else LIB_MLLVM[2:]) + ["-Wno-unused-value", "-fPIC", "-shared"] + \
          list(extra) + ["-D" + d for d in defines] + [SRC, "-L/opt/rocm/lib", "-lrccl"]
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    if "LMPC_NO_ISA_CHECK" in defines:                 # (developer flavours that WANT the faulty build: tools/n40_experiments.py)
        subprocess.check_call(cmd + ["-o", out])
        return out
    return compile_checked(cmd, out, verbose)


def build_asan():
    """The memory-safety flavour: liblmpc_hip_asan.so -- host side under AddressSanitizer, guard zones behind every device buffer (-DLMPC_GUARD)."""
    return build_flavour("asan", ["LMPC_GUARD"], extra=ASAN_FLAGS)


def build_guard():
    """Guard zones only (no AddressSanitizer): liblmpc_hip_guard.so -- the same device-buffer overrun check at full speed, with libstdc++ assertions on."""
    return build_flavour("guard", ["LMPC_GUARD", "_GLIBCXX_ASSERTIONS"])


def build(force=False, verbose=False):
    if not force and _current():
        return OUT
    import fcntl
    with open(OUT + ".lock", "w") as lock:             # several ranks may call build() at once: one compiles, the others wait
        fcntl.flock(lock, fcntl.LOCK_EX)
        if force or not _current():
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17"] + LIB_MLLVM + ["-Wno-unused-value", "-fPIC", "-shared", SRC,
                   "-L/opt/rocm/lib", "-lrccl"]
            if verbose:
                cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
            compile_checked(cmd, OUT, verbose)
    return OUT


def variant_path(N, S):
    return os.path.join(_HERE, "liblmpc_var_N%d_S%d.so" % (N, S))


def build_variant(N, S, force=False):
    """One (N, numSS_points) instantiation of the solve kernels as liblmpc_var_N<N>_S<S>.so (csrc/lmpc_variant.hip); 20 s of hipcc at the reference's sizes, minutes
    at N = 64.  The one-wave layout of every pair of the range fits a CU (108 KB of LDS per QP at N = 64 with 384 points); the two- and four-wave kernels are part of
    the object only where their layout fits the 160 KB as well (not at N = 64 from 96 points or N = 40 at 384: such a pair runs one wave per QP at every batch size).
    Raises RuntimeError where no code-generation option gives a build that passes the ISA check (compile_checked); Context() then tries the runtime kernel, whose layout
    does not fit a CU at N = 64 beyond 146 points or N = 40 beyond 366 -- such a pair would be refused with LMPC_E_ARG.  Of these only the pairs build() prepares and the
    GPU tests run -- (40, 384), (64, 192), (64, 384) -- are known to build; the other (N, numSS_points) with N from 37 and wide safe sets have not been compiled."""
    N, S = int(N), int(S)
    if not (2 <= N <= 64 and 0 <= S <= 384):
        raise ValueError("solve kernels exist for 2 <= N <= 64 and 0 <= numSS_points <= 384 (got N=%d, numSS_points=%d)" % (N, S))
    out = variant_path(N, S)
    deps = [VSRC] + KDEPS
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    import fcntl
    with open(out + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if force or not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            compile_checked([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-Wno-unused-value", "-fPIC", "-shared",
                             "-DLMPC_VARIANT_TU", "-DLMPC_VAR_N=%d" % N, "-DLMPC_VAR_S=%d" % S, VSRC], out, salts=VARIANT_SALTS)
    return out


def build_all(force=False, variants=None, jobs=None):
    """The library plus the extra variants, compiled concurrently (one hipcc process each)."""
    from concurrent.futures import ThreadPoolExecutor
    todo = list(EXTRA_VARIANTS if variants is None else variants)
    with ThreadPoolExecutor(max_workers=jobs or min(8, (os.cpu_count() or 2))) as ex:
        futs = [ex.submit(build, force)] + [ex.submit(build_variant, n, s, force) for n, s in todo]
        if variants is None:                       # the opt-in flavour tests/test_gpu_condensed.py runs against: kept current with the kernels it shares
            futs.append(ex.submit(build_flavour, "cd", ["LMPC_WITH_CD"]))
        return [f.result() for f in futs]


if __name__ == "__main__":
    print(build(force=True, verbose=True))
