"""Build libspx_hip.so (hipcc, gfx950 only) in-tree.  `python -m scaleprotoseg_amd.build`"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libspx_hip.so")
SOURCES = ["spx_api.hip", "spx_fwd_npb2.hip", "spx_fwd_npb4.hip", "spx_fwd_npb6.hip", "spx_bwd_npb2.hip", "spx_bwd_npb4.hip",
           "spx_bwd_npb6.hip", "spx_bank.hip", "spx_pack.hip", "spx_push.hip", "spx_prune.hip", "spx_eval.hip", "spx_kld.hip", "spx_ce.hip", "spx_gemm.hip",
           "spx_reg.hip", "spx_actloss.hip", "spx_overlap.hip", "spx_pushbox.hip", "spx_explain.hip", "spx_simplex.hip", "spx_masked_select.hip",
           "spx_nearest.hip", "spx_scale_agg.hip", "spx_parts.hip", "spx_batch.hip", "spx_msc.hip"]
HEADERS = ["spx_common.h", "spx_kld_walk.h", "spx_planes.h", "spx_overlap_sample.h", "spx_args.h", "spx_mainloop.h", "spx_fwd_impl.h", "spx_bwd_impl.h", os.path.join("..", "..", "include", "spx_hip.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]
FLAGS += os.environ.get("SPX_EXTRA_HIPCC_FLAGS", "").split()


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the MI355X extension cannot be built")
    return exe


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    hipcc = _hipcc()
    objdir = os.path.join(CSRC, "build")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        if force or _stale(o, [s] + hdrs):
            jobs.append([hipcc, *FLAGS, "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(objdir, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
