"""CPU tests (no GPU needed) of the policy-rollout library: libpikazoo_rollout.so exports its header's symbols and carries the
tree's build id, it is the last entry of the tuple ``build()`` / ``needs_build()`` / ``DEPS`` walk while the four older tuples
keep their lengths and contents, nothing loads it before its first use, its code object holds exactly six kernels without
scratch, the entry point refuses bad arguments before any launch and in the header's order, ``rollout_policy`` raises
``ValueError`` for everything out of scope before it needs the library, and -- on the C oracle alone -- the GPU test's
terminating cases do end games before the last slab of TERMINATING_K steps and play on behind them."""
import re
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest

import policy_rollout_cases as RC
from test_cabi_and_host import dynamic_pz_symbols, header_functions
from test_net_host import declared_arguments

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
NAMES = ["pz_rollout_abi_version", "pz_rollout_build_id", "pz_rollout_policy"]
KERNELS = sorted(f"pz_rollout::rollout_policy_kernel<{h}, {act}>" for h in (32, 64, 128) for act in (0, 1))


@pytest.fixture(scope="module")
def pz_build():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build

    build.build()
    return build


@pytest.fixture(scope="module")
def lib(pz_build):
    from pikazoo_amd import rollout

    return rollout.load()


def test_rollout_library_exports_exactly_its_header(pz_build, lib):
    from pikazoo_amd import _native, rollout

    assert header_functions("pikazoo_rollout.h") == NAMES == sorted(rollout.SIGNATURES) == dynamic_pz_symbols(pz_build.ROLLOUT_LIB)
    assert pz_build.library_id(pz_build.ROLLOUT_LIB) == pz_build.source_id() == lib.pz_rollout_build_id().decode()
    assert not pz_build.needs_build()
    assert lib.pz_rollout_abi_version() == rollout.ABI_VERSION == 1
    header = (REPO / "include" / "pikazoo_rollout.h").read_text()
    assert "#define PZ_ROLLOUT_ABI_VERSION 1" in header and f"#define PZ_ROLLOUT_MAX_STEPS (1 << 20)" in header and rollout.MAX_STEPS == 1 << 20
    # the sixteenth library is the new tuple's last entry; the four older tuples keep their lengths and contents
    assert len(pz_build.EVERY_TARGET) == 16 and pz_build.EVERY_TARGET[-1] == (pz_build.ROLLOUT_LIB, pz_build.ROLLOUT_SOURCES)
    assert pz_build.EVERY_TARGET[:15] == pz_build.LIBRARY_TARGETS
    assert len(pz_build.TARGETS) == 11 and len(pz_build.ALL_TARGETS) == 13 and len(pz_build.BUILD_TARGETS) == 14 and len(pz_build.LIBRARY_TARGETS) == 15
    assert pz_build.ALL_TARGETS[:11] == pz_build.TARGETS and pz_build.BUILD_TARGETS[:13] == pz_build.ALL_TARGETS
    assert pz_build.LIBRARY_TARGETS[:14] == pz_build.BUILD_TARGETS and pz_build.LIBRARY_TARGETS[14] == (pz_build.VTRACE_LIB, pz_build.VTRACE_SOURCES)
    assert [lib_path.name for lib_path, _ in pz_build.LIBRARY_TARGETS] == [
        "libpikazoo_hip.so", "libpikazoo_diag.so", "libpikazoo_learn.so", "libpikazoo_policy.so", "libpikazoo_ppo.so", "libpikazoo_net.so",
        "libpikazoo_netgrad.so", "libpikazoo_optim.so", "libpikazoo_batch.so", "libpikazoo_pool.so", "libpikazoo_league.so", "libpikazoo_act.so",
        "libpikazoo_pool_act.so", "libpikazoo_ego.so", "libpikazoo_vtrace.so"]
    assert pz_build.ROLLOUT_LIB not in [lib_path for lib_path, _ in pz_build.LIBRARY_TARGETS]
    for dep in (pz_build.ROLLOUT_SOURCES[0], pz_build.INCLUDE / "pikazoo_rollout.h", pz_build.CSRC / "pz_step_io.hpp", pz_build.CSRC / "pz_mlp_tile.hpp",
                pz_build.CSRC / "pz_policy_rows.hpp", pz_build.CSRC / "pz_physics.hpp"):
        assert dep in pz_build.DEPS and dep.exists(), dep
    for lib_path, _ in pz_build.EVERY_TARGET:
        assert pz_build.library_id(lib_path) == pz_build.source_id(), lib_path
    # no other library holds the entry point, and the product's ABI did not move
    for other, _ in pz_build.LIBRARY_TARGETS:
        assert not set(NAMES) & set(dynamic_pz_symbols(other)), other
    assert not set(NAMES) & set(_native.exported_names()) and _native.load().pz_abi_version() == 10
    # the binding's signature has the header's arguments
    args = declared_arguments(re.sub(r"/\*.*?\*/", "", header, flags=re.S), "pz_rollout_policy")
    assert len(args) == 42 == len(rollout.SIGNATURES["pz_rollout_policy"][1]) and list(CALL) == args


def test_the_helper_move_left_one_definition_of_each_helper():
    """the game I/O helpers live in csrc/pz_step_io.hpp alone, and both translation units include it"""
    kernels = (REPO / "pika-zoo_amd" / "csrc" / "pz_kernels.hip").read_text()
    shared = (REPO / "pika-zoo_amd" / "csrc" / "pz_step_io.hpp").read_text()
    for text in ("struct StateIO {", "void load_game(Game& g, const StateIO& io)", "void store_game(const Game& g, const StateIO& io",
                 "void stage_obs(const Game& g", "Rewards shape_rewards(const pz_config& cfg", "struct StatsIO {", "void stats_update(EpisodeStats& st",
                 "RngId make_rng_id(const pz_config& cfg"):
        assert text in shared and text not in kernels, text
    assert '#include "pz_step_io.hpp"' in kernels
    assert '#include "pz_step_io.hpp"' in (REPO / "pika-zoo_amd" / "csrc" / "pz_rollout.hip").read_text()


def test_importing_the_older_modules_does_not_load_the_rollout_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import pikazoo_amd; "
            "from pikazoo_amd import env, pikazoo_v0, learn, policy, ppo, net, netgrad, optim, batch, pool, league, act; "
            "assert 'pikazoo_amd.rollout' not in sys.modules; m = net.ActorCritic(); m.rollout; env.raw_env.rollout_policy; "
            "assert 'pikazoo_amd.rollout' not in sys.modules; import pikazoo_amd as p; assert 'rollout' in p.__all__; "
            "p.rollout.policy_rollout; assert 'pikazoo_amd.rollout' in sys.modules and p.rollout._lib is None; "
            "assert not any('libpikazoo_rollout' in line for line in open('/proc/self/maps')); print('ok')")
    r = subprocess.run([sys.executable, "-c", code, str(REPO / "pika-zoo_amd")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kernel_census_of_the_rollout_library(pz_build):
    """hidden width and activation are the compile-time choices: 3 x 2 kernels and nothing else; none uses scratch or spills a
    vector register; the LDS is dynamic; a wave (one per SIMD) stays inside the 512 registers it can have"""
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.fail("llvm-objdump of the ROCm toolchain is needed for the census")
    table = kernel_digest.kernels(pz_build.ROLLOUT_LIB)
    assert sorted(name for name in table if not name.endswith(".kd")) == KERNELS
    notes = kernel_notes.notes(pz_build.ROLLOUT_LIB)
    assert sorted(name.replace("void ", "").split("(")[0] for name, _ in notes) == KERNELS
    for name, row in notes:
        assert row[".private_segment_fixed_size"] == 0 and row[".vgpr_spill_count"] == 0, (name, row)
        assert row[".group_segment_fixed_size"] == 0, (name, row)
        assert row[".vgpr_count"] + row.get(".agpr_count", 0) <= 512, (name, row)
        print(name, {k: row[k] for k in (".vgpr_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count") if k in row},
              "instructions", table[name.replace("void ", "").split("(")[0]][1])


def test_the_lds_figures_of_the_header_and_the_binding():
    from pikazoo_amd import rollout

    header = re.sub(r"\s+\*\s+", " ", (REPO / "include" / "pikazoo_rollout.h").read_text())
    for hidden, sets, fits in ((128, 2, False), (128, 1, True), (64, 2, True), (64, 1, True), (32, 2, True)):
        need = rollout.lds_bytes(hidden, 19, sets)
        assert (need <= rollout.LDS_BYTES) == fits, (hidden, sets, need)
        if hidden >= 64:
            assert f"{need:,}".replace(",", " ") + " B" in header, (hidden, sets, need)
    assert rollout.LDS_BYTES == 163840 and "163 840 B" in header


FAKE = 4096


def config(**over):
    from pikazoo_amd import _native

    cfg = _native.PzConfig()
    cfg.winning_score, cfg.x_line, cfg.y_line, cfg.auto_reset = 15, 216, 176, 1
    for key, value in over.items():
        setattr(cfg, key, value)
    return cfg


CALL = dict(state=FAKE, n=8, stride=64, cfg=None, k=4, hidden=64, out_features=19, activation=0, w1_p1=FAKE, b1_p1=FAKE, w2_p1=FAKE,
            b2_p1=FAKE, w3_p1=FAKE, b3_p1=FAKE, w1_p2=None, b1_p2=None, w2_p2=None, b2_p2=None, w3_p2=None, b3_p2=None, seed=7,
            first_game=0, step=0, step_dev=None, action_format=1, pitch=8, obs_p1=FAKE, obs_p2=FAKE, act_p1=FAKE, act_p2=FAKE,
            logp_p1=FAKE, logp_p2=FAKE, val_p1=FAKE, val_p2=FAKE, ent_p1=FAKE, ent_p2=FAKE, rew_p1=FAKE, rew_p2=FAKE, terminated=FAKE,
            episode_stats=None, episodes_done=None, stream=None)
SET_2 = ["w1_p2", "b1_p2", "w2_p2", "b2_p2", "w3_p2", "b3_p2"]


def test_argument_validation(lib):
    """every return code on fake pointers, in the order the header lists them: a call that passes every check has n = 0 and
    launches nothing"""
    import ctypes as C

    def call(cfg=None, **over):
        a = dict(CALL)
        assert not set(over) - set(a)
        a.update(over)
        keep = cfg if cfg is not None else config()
        a["cfg"] = C.byref(keep)
        return lib.pz_rollout_policy(*a.values())

    own = {name: FAKE + 1024 for name in SET_2}
    assert call(n=0, pitch=0) == 0 and call(n=0, pitch=0, **own) == 0
    # PZ_E_NULL: required pointers, agent 2's parameters all or none, the entropy pair together
    required = ["state", "w1_p1", "b1_p1", "w2_p1", "b2_p1", "w3_p1", "b3_p1", "obs_p1", "obs_p2", "act_p1", "act_p2", "logp_p1", "logp_p2",
                "val_p1", "val_p2", "rew_p1", "rew_p2", "terminated"]
    for name in required:
        assert call(**{name: None}) == -1, name
    assert lib.pz_rollout_policy(*{**CALL, "cfg": None}.values()) == -1
    for name in SET_2:
        assert call(**{name: FAKE}) == -1, name
        assert call(**{**own, name: None}) == -1, name
    assert call(ent_p1=None) == -1 and call(ent_p2=None) == -1 and call(n=0, pitch=0, ent_p1=None, ent_p2=None) == 0
    assert call(n=0, pitch=0, episode_stats=FAKE, episodes_done=FAKE, step_dev=FAKE) == 0
    # PZ_E_SIZE: sizes, pitches and steps beyond range
    limit = 0xFFFFFFFF // 176
    assert call(n=-1) == -2 and call(n=9, stride=8, pitch=9) == -2 and call(stride=limit + 1) == -2 and call(n=0, pitch=0, stride=limit) == 0
    assert call(k=0) == -2 and call(k=-3) == -2 and call(k=(1 << 20) + 1) == -2 and call(n=0, pitch=0, k=1 << 20) == 0
    for hidden in (0, 16, 33, 96, 256, -64):
        assert call(hidden=hidden) == -2, hidden
    assert call(n=0, pitch=0, hidden=32) == 0 and call(n=0, pitch=0, hidden=128) == 0
    for out_features in (18, 20, 14, 0, 40):
        assert call(out_features=out_features) == -2, out_features
    assert call(config(simplify_action=1), out_features=19) == -2 and call(config(simplify_action=1), n=0, pitch=0, out_features=14) == 0
    assert call(pitch=7) == -2 and call(pitch=limit + 1) == -2 and call(n=0, pitch=limit) == 0 and call(n=0, pitch=12) == 0
    assert call(first_game=-1) == -2 and call(n=0, pitch=0, first_game=(1 << 62)) == 0
    assert call(step=(1 << 62) - 3) == -2 and call(step=1 << 63) == -2 and call(n=0, pitch=0, step=(1 << 62) - 4) == 0
    # PZ_E_CONFIG: configuration enums, what is out of scope, unknown formats
    for bad in (dict(winning_score=0), dict(serve_mode=3), dict(normal_state_mode=3), dict(episode_stats_mode=-1), dict(normalize_obs=7),
                dict(packed_state=2), dict(p1_computer=1), dict(p2_computer=1), dict(packed_state=1), dict(normalize_obs=2), dict(normalize_obs=5)):
        assert call(config(**bad)) == -3, bad
    for good in (dict(normalize_obs=1), dict(auto_reset=0), dict(ballpos_reward=1), dict(normal_state_mode=2), dict(episode_stats_mode=2), dict(serve_mode=2)):
        assert call(config(**good), n=0, pitch=0) == 0, good
    for name, count in (("activation", 2), ("action_format", 2)):
        assert call(**{name: count}) == -3 and call(**{name: -1}) == -3, name
        for value in range(count):
            assert call(n=0, pitch=0, **{name: value}) == 0, (name, value)
    # PZ_E_ALIGN: every pointer to its element
    for name in [k for k in CALL if k.endswith(("_p1", "_p2"))] + ["state"]:
        base = own if name in SET_2 else {}
        assert call(**{**base, name: FAKE + 1}) == -4 and call(**{**base, name: FAKE + 2}) == -4, name
        if name.startswith("act"):
            assert call(**{name: FAKE + 4}) == -4 and call(n=0, pitch=0, action_format=0, **{name: FAKE + 4}) == 0, name
        else:
            assert call(n=0, pitch=0, **{**base, name: FAKE + 4}) == 0, name
    for name in ("episode_stats", "episodes_done", "step_dev"):
        assert call(**{name: FAKE + 4}) == -4 and call(n=0, pitch=0, **{name: FAKE + 8}) == 0, name
    # the LDS refusal: hidden 128 with a parameter set per agent -- behind the alignment check, in front of n == 0
    assert call(n=0, pitch=0, hidden=128, **own) == -2 and call(hidden=128, **own) == -2
    assert call(n=0, pitch=0, hidden=128, **{name: FAKE for name in SET_2}) == 0          # (agent 1's pointers again: one set)
    assert call(n=0, pitch=0, hidden=64, **own) == 0 and call(n=0, pitch=0, hidden=32, **own) == 0
    assert call(hidden=128, act_p1=FAKE + 2, **own) == -4
    # the order of the checks: NULL, size, config, alignment, LDS
    assert call(config(p1_computer=1), b3_p1=None, n=-1, act_p1=FAKE + 2) == -1
    assert call(config(p1_computer=1), n=-1, act_p1=FAKE + 2) == -2
    assert call(config(p1_computer=1), act_p1=FAKE + 2) == -3
    assert call(activation=9, act_p1=FAKE + 2) == -3
    assert call(act_p1=FAKE + 2) == -4


def stub_env(**over):
    """what rollout.policy_rollout reads of an env before it launches"""
    import torch

    from pikazoo_amd import _native

    env = types.SimpleNamespace(_mixed=False, _cfg=_native.PzConfig(), frame_skip=1, state_format="int32", _unfused=[], obs_dtype=torch.int32,
                                possible_agents=["player_1", "player_2"], num_envs=8, device=torch.device("cpu"), n_actions=18)
    for key, value in over.items():
        if key.startswith("cfg_"):
            setattr(env._cfg, key[4:], value)
        else:
            setattr(env, key, value)
    return env


def test_python_errors_come_before_the_library_is_needed(monkeypatch):
    """everything the launch does not take raises ValueError naming the limit, and so do malformed arguments; none of them asks
    for the library (on a CPU stand-in for the env the device check stands behind the others)"""
    import torch

    from pikazoo_amd import net, pool, rollout

    def refuse():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(rollout, "load", refuse)
    model = net.ActorCritic()
    run = lambda env=None, params=model, k=4, **kw: rollout.policy_rollout(env or stub_env(), params, k, kw.pop("seed", 1), **kw)  # noqa: E731
    with pytest.raises(ValueError, match="GPU"):
        run()
    with pytest.raises(ValueError, match="GPU"):
        run(params={"player_1": model, "player_2": net.ActorCritic()}, entropy=True, action_dtype=torch.int32, step=5)
    # out of scope
    for over, words in ((dict(_mixed=True), "mixed"), (dict(cfg_p1_computer=1), "computer"), (dict(cfg_p2_computer=1), "computer"),
                        (dict(frame_skip=4), "frame_skip"), (dict(state_format="packed"), "packed"),
                        (dict(cfg_normalize_obs=2, obs_dtype=torch.int16), "2-byte"), (dict(cfg_normalize_obs=5, obs_dtype=torch.float16), "2-byte"),
                        (dict(_unfused=["RewardByBallPosition"]), "outside the kernel")):
        with pytest.raises(ValueError, match=words):
            run(stub_env(**over))
    with pytest.raises(ValueError, match="pool"):
        run(params=pool.Snapshots.__new__(pool.Snapshots))
    # the LDS refusal, the net's shape against the env's actions
    with pytest.raises(ValueError, match="LDS"):
        run(params={"player_1": net.ActorCritic(hidden=128), "player_2": net.ActorCritic(hidden=128)})
    with pytest.raises(ValueError, match="GPU"):
        run(params=net.ActorCritic(hidden=128))
    with pytest.raises(ValueError, match="GPU"):
        shared = net.ActorCritic(hidden=128)
        run(params={"player_1": shared, "player_2": shared})
    with pytest.raises(ValueError, match="14 outputs"):
        run(stub_env(n_actions=13))
    with pytest.raises(ValueError, match="GPU"):
        run(stub_env(n_actions=13), params=net.ActorCritic(num_actions=13))
    good = [p.data for p in model.parameter_tensors()]
    bad_calls = [dict(params=good[:5]), dict(params={"player_2": model, "player_1": model}), dict(params={"player_1": model}),
                 dict(params=[torch.zeros(48, 35)] + good[1:]), dict(params=[torch.zeros(64, 36)] + good[1:]), dict(k=0), dict(k=(1 << 20) + 1),
                 dict(env=stub_env(num_envs=6), k=2), dict(seed=-1), dict(seed=1 << 64), dict(first_game=-1), dict(first_game=1 << 62),
                 dict(step=-1), dict(step=(1 << 62) - 3), dict(step=torch.zeros(2, dtype=torch.int64)), dict(step=torch.zeros(1, dtype=torch.int32)),
                 dict(action_dtype=torch.int16), dict(activation="gelu", params=good), dict(out={}), dict(out=torch.zeros(4)),
                 dict(out={"_policy": (5, 8, torch.int64, False)})]
    for bad in bad_calls:
        with pytest.raises(ValueError):
            run(**bad)
    with pytest.raises(ValueError, match="GPU"):
        run(env=stub_env(num_envs=6), k=1)           # (one step: any batch size)
    with pytest.raises(ValueError, match="GPU"):
        run(params=good, activation="relu", first_game=(1 << 62) - 1, step=(1 << 62) - 4)


@pytest.mark.parametrize("n,auto_reset", RC.TERMINATING_CASES)
def test_games_end_inside_a_launch_of_the_terminating_k(oracle, n, auto_reset):
    """On the C oracle alone, under uniformly random actions from a fixed numpy seed (a proxy for the sampled ones): at the
    GPU test's terminating cases a game ends at a slab t < k - 1, and with auto_reset it plays on inside the launch -- its flag
    comes down with the next frame and its state moves again; without, it stays frozen and its flag stays up"""
    k = RC.TERMINATING_K
    term, moved_after = RC.proxy_play(n, auto_reset)
    first = np.where(term.any(0), term.argmax(0), k)
    early = first < k - 1
    print(f"n = {n}, auto_reset = {auto_reset}, k = {k}: {int(early.sum())} games end before the last slab, the first at t = {int(first.min())}; "
          f"{int((term.sum(0) > 1).sum())} games raise the flag more than once")
    assert k == 32 and early.sum() >= n // 8
    if auto_reset:
        assert (moved_after[early] > 0).all()
        for g in np.nonzero(early)[0]:
            assert term[first[g] + 1, g] == 0   # reset in place and playing: a rally cannot end with its first frame
    else:
        assert (moved_after == 0).all()
        for g in np.nonzero(early)[0]:
            assert term[first[g]:, g].all()
