"""Build libpikazoo_hip.so -- and beside it libpikazoo_diag.so, libpikazoo_learn.so, libpikazoo_policy.so,
libpikazoo_ppo.so, libpikazoo_net.so, libpikazoo_netgrad.so, libpikazoo_optim.so, libpikazoo_batch.so, libpikazoo_pool.so,
libpikazoo_league.so, libpikazoo_act.so, libpikazoo_pool_act.so, libpikazoo_ego.so, libpikazoo_vtrace.so and libpikazoo_rollout.so -- for gfx950 with hipcc (in-tree, no JIT cache).

    python pika-zoo_amd/build.py [--force]

The product library is plain HIP + a C ABI (include/pikazoo_hip.h); it links only against the
HIP runtime, not against torch.  hipcc cross-compiles without a GPU present.  The diagnostics library
(include/pikazoo_diag.h: pz_probe_launch, pz_selftest_predictor) is compiled from the product's own headers and is
loaded by bench.py and tests/ only (pika-zoo_amd/diag.py); it carries the same build id.  The learning library
(include/pikazoo_learn.h: pz_gae) is a third translation unit with kernels of its own, bound by pikazoo_amd/learn.py; the
product library holds none of it.  The policy library (include/pikazoo_policy.h: pz_sample_actions, pz_action_log_probs and
its backward) is a fourth, bound by pikazoo_amd/policy.py; the PPO library (include/pikazoo_ppo.h: pz_ppo_moments, pz_ppo_loss)
a fifth, bound by pikazoo_amd/ppo.py, which shares csrc/pz_policy_rows.hpp with the fourth; the net library
(include/pikazoo_net.h: pz_mlp_forward) a sixth, bound by pikazoo_amd/net.py; the net-gradient library
(include/pikazoo_netgrad.h: pz_mlp_backward) a seventh, bound by pikazoo_amd/netgrad.py; the optimizer library
(include/pikazoo_optim.h: pz_adam_step) an eighth, bound by pikazoo_amd/optim.py; the batch library
(include/pikazoo_batch.h: pz_batch_copy, pz_batch_gather) a ninth, bound by pikazoo_amd/batch.py; the pool library
(include/pikazoo_pool.h: pz_pool_plan, pz_mlp_forward_pool) a tenth, bound by pikazoo_amd/pool.py, which shares its tile
code (csrc/pz_mlp_tile.hpp) with the sixth; the league library (include/pikazoo_league.h: pz_league_tally, pz_league_draw) an
eleventh, bound by pikazoo_amd/league.py; the act library (include/pikazoo_act.h: pz_mlp_act) a twelfth, bound by
pikazoo_amd/act.py, which shares csrc/pz_mlp_tile.hpp with the sixth and csrc/pz_policy_rows.hpp with the fourth; the pool-act library
(include/pikazoo_pool_act.h: pz_mlp_act_pool) a thirteenth, bound by pikazoo_amd/pool_act.py, which shares both headers with the
twelfth; the ego library (include/pikazoo_ego.h: pz_ego_rows, pz_ego_actions) a fourteenth, bound by pikazoo_amd/ego.py; the
V-trace library (include/pikazoo_vtrace.h: pz_vtrace) a fifteenth, bound by pikazoo_amd/vtrace.py, which shares its scan over
the trajectory (csrc/pz_traj_scan.hpp) with the third; the rollout library (include/pikazoo_rollout.h: pz_rollout_policy) a
sixteenth, bound by pikazoo_amd/rollout.py, which shares the frame and its I/O (csrc/pz_physics.hpp, csrc/pz_step_io.hpp) with the
first, csrc/pz_mlp_tile.hpp with the sixth and csrc/pz_policy_rows.hpp with the fourth.  The sixteen compiles are independent and
run side by side.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parent
REPO = PKG_ROOT.parent
CSRC = PKG_ROOT / "csrc"
INCLUDE = REPO / "include"
LIB_DIR = PKG_ROOT / "lib"
LIB = LIB_DIR / "libpikazoo_hip.so"
DIAG_LIB = LIB_DIR / "libpikazoo_diag.so"
LEARN_LIB = LIB_DIR / "libpikazoo_learn.so"
POLICY_LIB = LIB_DIR / "libpikazoo_policy.so"
PPO_LIB = LIB_DIR / "libpikazoo_ppo.so"
NET_LIB = LIB_DIR / "libpikazoo_net.so"
NETGRAD_LIB = LIB_DIR / "libpikazoo_netgrad.so"
OPTIM_LIB = LIB_DIR / "libpikazoo_optim.so"
BATCH_LIB = LIB_DIR / "libpikazoo_batch.so"
POOL_LIB = LIB_DIR / "libpikazoo_pool.so"
LEAGUE_LIB = LIB_DIR / "libpikazoo_league.so"
ACT_LIB = LIB_DIR / "libpikazoo_act.so"
POOL_ACT_LIB = LIB_DIR / "libpikazoo_pool_act.so"
EGO_LIB = LIB_DIR / "libpikazoo_ego.so"
VTRACE_LIB = LIB_DIR / "libpikazoo_vtrace.so"
ROLLOUT_LIB = LIB_DIR / "libpikazoo_rollout.so"
SOURCES = [CSRC / "pz_kernels.hip"]
DIAG_SOURCES = [CSRC / "pz_diag.hip"]
LEARN_SOURCES = [CSRC / "pz_learn.hip"]
POLICY_SOURCES = [CSRC / "pz_policy.hip"]
PPO_SOURCES = [CSRC / "pz_ppo.hip"]
NET_SOURCES = [CSRC / "pz_net.hip"]
NETGRAD_SOURCES = [CSRC / "pz_netgrad.hip"]
OPTIM_SOURCES = [CSRC / "pz_optim.hip"]
BATCH_SOURCES = [CSRC / "pz_batch.hip"]
POOL_SOURCES = [CSRC / "pz_pool.hip"]
LEAGUE_SOURCES = [CSRC / "pz_league.hip"]
ACT_SOURCES = [CSRC / "pz_act.hip"]
POOL_ACT_SOURCES = [CSRC / "pz_pool_act.hip"]
EGO_SOURCES = [CSRC / "pz_ego.hip"]
VTRACE_SOURCES = [CSRC / "pz_vtrace.hip"]
ROLLOUT_SOURCES = [CSRC / "pz_rollout.hip"]
# every library with the translation units it is compiled from
TARGETS = ((LIB, SOURCES), (DIAG_LIB, DIAG_SOURCES), (LEARN_LIB, LEARN_SOURCES), (POLICY_LIB, POLICY_SOURCES), (PPO_LIB, PPO_SOURCES),
           (NET_LIB, NET_SOURCES), (NETGRAD_LIB, NETGRAD_SOURCES), (OPTIM_LIB, OPTIM_SOURCES), (BATCH_LIB, BATCH_SOURCES),
           (POOL_LIB, POOL_SOURCES), (LEAGUE_LIB, LEAGUE_SOURCES))
# ... and the libraries added since (TARGETS keeps its eleven entries, ALL_TARGETS its thirteen)
ALL_TARGETS = TARGETS + ((ACT_LIB, ACT_SOURCES), (POOL_ACT_LIB, POOL_ACT_SOURCES))
# ... and the ego library (BUILD_TARGETS keeps its fourteen)
BUILD_TARGETS = ALL_TARGETS + ((EGO_LIB, EGO_SOURCES),)
# ... and the V-trace library (LIBRARY_TARGETS keeps its fifteen)
LIBRARY_TARGETS = BUILD_TARGETS + ((VTRACE_LIB, VTRACE_SOURCES),)
# what build(), needs_build() and DEPS walk: every library there is
EVERY_TARGET = LIBRARY_TARGETS + ((ROLLOUT_LIB, ROLLOUT_SOURCES),)
DEPS = [source for _, sources in EVERY_TARGET for source in sources] + [
    CSRC / "pz_physics.hpp", CSRC / "pz_packed.hpp", CSRC / "pz_memory.hpp", CSRC / "pz_step_io.hpp", CSRC / "pz_diagnostic.hpp", CSRC / "pz_dispatch.hpp",
    CSRC / "pz_policy_rows.hpp", CSRC / "pz_mlp_tile.hpp", CSRC / "pz_traj_scan.hpp", INCLUDE / "pikazoo_hip.h", INCLUDE / "pikazoo_diag.h", INCLUDE / "pikazoo_learn.h",
    INCLUDE / "pikazoo_policy.h", INCLUDE / "pikazoo_ppo.h", INCLUDE / "pikazoo_net.h", INCLUDE / "pikazoo_netgrad.h",
    INCLUDE / "pikazoo_optim.h", INCLUDE / "pikazoo_batch.h", INCLUDE / "pikazoo_pool.h", INCLUDE / "pikazoo_league.h", INCLUDE / "pikazoo_act.h",
    INCLUDE / "pikazoo_pool_act.h", INCLUDE / "pikazoo_ego.h", INCLUDE / "pikazoo_vtrace.h", INCLUDE / "pikazoo_rollout.h"]
ARCH = "gfx950"
# the step kernels' six leading arguments (11 dwords) are preloaded into SGPRs at wave launch (pz_kernels.hip: HotArgs)
FLAGS = ["-O3", "-std=c++17", f"--offload-arch={ARCH}", "-mllvm", "-amdgpu-kernarg-preload-count=11"]


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


def source_id(extra_flags=()) -> str:
    """Digest of the sources and compiler flags the library is built from; baked into the library as
    ``pz_build_id()`` so that a stale prebuilt .so (git-ignored, but shipped to the GPU box) is never run.
    `extra_flags` are part of it: a variant compiled with other flags and copied to the product path carries
    another id than the product and is refused by ``_native.load()`` / rebuilt by ``needs_build()``."""
    h = hashlib.sha256()
    for d in DEPS:
        h.update(d.name.encode() + b"\0" + d.read_bytes() + b"\0")
    h.update(" ".join([*FLAGS, *extra_flags]).encode())
    return h.hexdigest()[:16]


_ID_MARKER = b"pz_build_id:"


def library_id(lib: Path = LIB):
    """The build id baked into a built library, or None (missing file / pre-build-id library).  Read from
    the file's bytes (the library stores it behind the marker ``pz_build_id:``), not through dlopen: a
    stale library mapped into this process would shadow the rebuilt one of the same name."""
    if not lib.exists():
        return None
    data = lib.read_bytes()
    at = data.find(_ID_MARKER)
    if at < 0:
        return None
    end = data.find(b"\0", at)
    return data[at + len(_ID_MARKER):end].decode(errors="replace")


def needs_build() -> bool:
    return any(library_id(lib) != source_id() for lib, _ in EVERY_TARGET)


def _compile(out: Path, sources, extra_flags, verbose: bool) -> None:
    # compile to a temporary name and rename: other ranks / processes never see a half-written library
    tmp = out.with_suffix(f".so.tmp{os.getpid()}")
    cmd = [hipcc_path(), *FLAGS, "-shared", "-fPIC", f'-DPZ_BUILD_ID="{source_id(tuple(extra_flags))}"',
           f"-I{INCLUDE}", f"-I{CSRC}", *extra_flags, "-o", str(tmp), *map(str, sources)]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, out)


def build(force: bool = False, verbose: bool = False, extra_flags=()) -> Path:
    """The product library (returned) with the diagnostics, the learning, the policy, the PPO, the net, the net-gradient, the
    optimizer, the batch, the pool, the league, the act, the pool-act, the ego, the V-trace and the rollout library beside it: each is compiled when it is missing or stale,
    the compiles side by side (a cold build takes about as long as the product library alone: some three minutes; an
    up-to-date tree costs sixteen file reads)."""
    if any("PZ_DIAGNOSTIC_BUILD" in f for f in extra_flags):
        # csrc/pz_diagnostic.hpp: the one compile-time switch of the kernels -- tools/ab.py builds such variants into
        # tools/bin/; the product path never holds one (and _native.load() would refuse its build id "diagnostic")
        raise ValueError("a diagnostic build (-DPZ_DIAGNOSTIC_BUILD) is never written to the product library's path")
    want = source_id(tuple(extra_flags))
    LIB_DIR.mkdir(parents=True, exist_ok=True)
    todo = [(out, sources) for out, sources in EVERY_TARGET if force or extra_flags or library_id(out) != want]
    if len(todo) > 1:
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(len(todo)) as pool:  # (the threads only wait for their hipcc)
            for done in [pool.submit(_compile, out, sources, extra_flags, verbose) for out, sources in todo]:
                done.result()
    elif todo:
        _compile(*todo[0], extra_flags, verbose)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
