"""Build libslow5gpu.so (HIP kernels + C ABI) in-tree for gfx950.  hipcc cross-compiles without a GPU."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libslow5gpu.so")
S5VIEW = os.path.join(HERE, "s5view")

HIP_SOURCES = ["encode_kernels.hip", "decode_kernels.hip", "batch_kernels.hip", "order_launch.hip", "host_api.hip", "ascii_kernels.hip", "ascii_api.hip", "skim_kernels.hip", "skim_api.hip", "signal_kernels.hip", "signal_api.hip", "digest_kernels.hip", "digest_api.hip", "fstats_kernels.hip", "fstats_api.hip", "diff_kernels.hip", "diff_api.hip", "event_kernels.hip", "event_api.hip", "dtw_kernels.hip", "dtw_api.hip", "dtw_path_kernels.hip", "dtw_path_api.hip", "pileup_kernels.hip", "pileup_api.hip", "refine_kernels.hip", "refine_api.hip", "refine_long_api.hip", "refine_long_kernels.hip", "band_kernels.hip", "band_api.hip", "contrast_kernels.hip", "contrast_api.hip", "sites_kernels.hip", "sites_api.hip", "fold_kernels.hip", "fold_api.hip"]
C_SOURCES = ["slow5_compat.c", "blow5_file.c", "refseq.c"]
DEPS = ["dev_common.h", "deflate_dev.h", "deflate2_dev.h", "lz_dev.h", "inflate_dev.h", "inflate_simt_dev.h", "inflate_par_dev.h", "svb_dev.h", "exzd_dev.h", "zstd_dev.h", "zstd_enc_dev.h", "host_ctx.h", "skim_dev.h", "signal_dev.h", "digest_dev.h", "fstats_dev.h", "diff_dev.h", "event_dev.h", "dtw_dev.h", "dtw_host.h", "pileup_dev.h", "ragged_dev.h", "pileup_host.h", "fold_dev.h", "sites_dev.h", "refine_dev.h", "refine_host.h", "band_dev.h", "band_host.h", "order_dev.h", "enc_plan.h", "dec_plan.h", "launch_common.h", "resident_rules.h", "event_host.h",
        os.path.join(ROOT, "include", "slow5gpu.h"), os.path.join(ROOT, "include", "slow5_compat.h"), os.path.join(ROOT, "include", "slow5gpu_hooks.h")]


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.exists(s) and os.path.getmtime(s) > t for s in sources)


def build(force=False, verbose=False):
    deps = [d if os.path.isabs(d) else os.path.join(CSRC, d) for d in DEPS]
    objs = []
    for src in HIP_SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", ".o"))
        if force or _newer(o, [s] + deps):
            # max-memory-clause: the scheduler groups memory operations; +5 % on the lane-per-record inflate kernel, neutral elsewhere
            cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-sched-strategy=max-memory-clause"]
            cmd += os.environ.get("S5_HIPCC_EXTRA", "").split() + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.check_call(cmd)
        objs.append(o)
    for src in C_SOURCES:
        s = os.path.join(CSRC, src)
        if not os.path.exists(s):
            continue
        o = os.path.join(CSRC, src.replace(".c", ".o"))
        if force or _newer(o, [s] + deps):
            cmd = ["gcc", "-O2", "-g", "-Wall", "-std=c11", "-fPIC", "-I", os.path.join(ROOT, "include"), "-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.check_call(cmd)
        objs.append(o)
    if force or _newer(LIB, objs):
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    # the view / get / merge / skim / sum / stats / diff / events / map / align / pileup / refine / extend / contrast / sites / model loop examples = the end-to-end harnesses (plain C against the public headers)
    tool_h = os.path.join(ROOT, "examples", "s5tool.h")    # what the tools share: each of them includes it
    for name in ("s5view", "s5get", "s5merge", "s5skim", "s5sum", "s5stats", "s5diff", "s5events", "s5map", "s5align", "s5pileup", "s5refine", "s5extend", "s5contrast", "s5sites", "s5model"):
        ex = os.path.join(ROOT, "examples", name + ".c")
        exe = os.path.join(HERE, name)
        if os.path.exists(ex) and (force or _newer(exe, [ex, tool_h, LIB] + deps)):
            cmd = ["gcc", "-O2", "-g", "-Wall", "-std=c11", "-I", os.path.join(ROOT, "include"), ex, "-o", exe, "-pthread",
                   "-L", HERE, "-lslow5gpu", "-lm", "-Wl,-rpath," + HERE]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
