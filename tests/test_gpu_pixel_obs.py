"""GPU tests of the pixel observations (``pz_render_gray``, ``raw_env.render_observations``,
``wrappers.PixelObservation``): grey, box-filtered frames == the definition of tests/pixel_judge.py on top of the numpy
frame oracle, bit for bit, at every scale, on synthetic sprites of the reference's geometry; 70 games (one full wave of
games and a tail of six)."""
import numpy as np
import pytest
import torch

import pixel_judge as pj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A1, A2 = "player_1", "player_2"


@pytest.fixture(scope="module")
def sprites():
    from pikazoo_amd.render import synthetic_sprites

    return synthetic_sprites(7, DEV)


def _env(sprites, **kw):
    from pikazoo_amd import pikazoo_v0

    args = dict(num_envs=pj.N, device=DEV, seed=4, render_mode="rgb_array", sprites=sprites, winning_score=15)
    args.update(kw)
    return pikazoo_v0.env(**args)


def _first_difference(got, want):
    l, y, x = np.argwhere(got != want)[0]
    return f"lane {l} pixel ({x},{y}): hip {got[l, y, x]} != judge {want[l, y, x]}"


@pytest.fixture(scope="module")
def played(sprites):
    """(env after 60 random steps, its state) and (env on the planted states, that state): shared, never stepped again."""
    env = _env(sprites, is_player1_computer=True, is_player2_computer=True)
    env.reset()
    env.step_random(3, k=60)
    planted = _env(sprites)
    planted.reset()
    planted.set_state(torch.from_numpy(pj.plant(planted.state.cpu().numpy(), pj.states())).to(DEV))
    return (env, env.state.cpu().numpy()), (planted, planted.state.cpu().numpy())


@pytest.mark.parametrize("scale", pj.SCALES)
def test_frames_match_the_judge(played, sprites, scale):
    from oracle import render_oracle as ro

    P2 = ro.P_WORDS
    for env, st in played:
        got = env.render_observations(scale)
        assert got.shape == (pj.N, 304 // scale, 432 // scale) and got.dtype == torch.uint8 and got.device.type == "cuda"
        got, want = got.cpu().numpy(), pj.frames(st, sprites, scale)
        assert np.array_equal(got, want), _first_difference(got, want)
        assert np.array_equal(env.state.cpu().numpy(), st)
    st = played[1][1]  # the planted states: each situation is there
    dive1 = np.isin(st[ro.P_STATE], (3, 4)) & (st[ro.P_DIVE] == -1)
    dive2 = np.isin(st[P2 + ro.P_STATE], (3, 4)) & (st[P2 + ro.P_DIVE] == 1)
    seen = {"power": (st[ro.B_POWER] != 0).sum(), "mirrored dive of player 1": dive1.sum(),
            "unmirrored dive of player 2": dive2.sum(), "scores >= 10": ((st[ro.E_S1] >= 10) & (st[ro.E_S2] >= 10)).sum(),
            "ball at the top": (st[ro.B_Y] < 20).sum(), "ball at the left": (st[ro.B_X] < 20).sum(),
            "ball at the right": (st[ro.B_X] > 412).sum(), "ball at the bottom": (st[ro.B_Y] > 284).sum(),
            "diver at the left wall": (np.isin(st[ro.P_STATE], (3, 4)) & (st[ro.P_X] < 32)).sum(),
            "diver at the right wall": (np.isin(st[P2 + ro.P_STATE], (3, 4)) & (st[P2 + ro.P_X] > 400)).sum()}
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("scale", pj.SCALES)
def test_lanes_and_a_slot_of_a_frame_stack(played, sprites, scale):
    env, st = played[1]
    lanes = [69, 3, 64, 0, 3, 10, 65, 7]  # arbitrary order, one repeated, both sides of the wave boundary
    h, w = 304 // scale, 432 // scale
    big = torch.full((len(lanes), 3, h, w), 0xA5, dtype=torch.uint8, device=DEV)
    out = env.render_observations(scale, lanes=lanes, out=big[:, 1])
    assert out.data_ptr() == big[:, 1].data_ptr()
    got = big.cpu().numpy()
    want = pj.frames(st, sprites, scale, lanes)
    assert np.array_equal(got[:, 1], want), _first_difference(got[:, 1], want)
    assert (got[:, 0] == 0xA5).all() and (got[:, 2] == 0xA5).all()
    assert np.array_equal(env.render_observations(scale, lanes=torch.tensor(lanes, device=DEV)).cpu().numpy(), want)
    with pytest.raises(IndexError):
        env.render_observations(scale, lanes=[pj.N])


@pytest.mark.parametrize("scale", pj.SCALES)
def test_with_and_without_the_grey_background(played, sprites, scale):
    from pikazoo_amd import render as R

    for env, _ in played:
        frames = []
        for fast in (True, False):
            with torch.cuda.device(env.device):
                frames.append(R.render_gray(env._lib, env._state_buf.data_ptr(), env.device, env.num_envs, env._stride, sprites,
                                            None, env._stream(), scale, fast_path=fast))
        assert torch.equal(frames[0], frames[1])
        assert torch.equal(frames[0], env.render_observations(scale))


def test_packed_state_env_draws_what_the_int32_env_draws(sprites):
    envs = [_env(sprites, state_format=fmt, is_player2_computer=True) for fmt in ("int32", "packed")]
    for e in envs:
        e.reset()
        e.step_random(5, k=45)
    assert torch.equal(envs[0].read_state(), envs[1].read_state())
    for scale in pj.SCALES:
        assert torch.equal(envs[0].render_observations(scale), envs[1].render_observations(scale))
    want = pj.frames(envs[1].read_state().cpu().numpy(), sprites, 4)
    assert np.array_equal(envs[1].render_observations(4).cpu().numpy(), want)


def test_an_observation_does_not_change_the_game(sprites):
    tape = torch.randint(0, 18, (20, 2, pj.N), dtype=torch.int32, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    runs = []
    for watched in (False, True):
        env = _env(sprites, is_player2_computer=True, seed=11)
        env.reset()
        env.step_random(2, k=30)
        if watched:
            for scale in pj.SCALES:
                env.render_observations(scale)
            env.render_observations(4, lanes=[1, 1, 5])
        state = env.read_state().clone()  # (word 43: the env RNG's draw counter)
        outs = []
        for t in range(20):
            obs, rew, term, _, _ = env.step({A1: tape[t, 0], A2: tape[t, 1]})
            if watched:
                env.render_observations(2)
            outs.append((obs[A1].clone(), obs[A2].clone(), rew[A1].clone(), term[A1].clone()))
        runs.append((state, outs, env.read_state().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_api_refusals(sprites, monkeypatch):
    from pikazoo_amd import pikazoo_v0
    from pikazoo_amd import render as R
    from pikazoo_amd.wrappers import PixelObservation

    with pytest.raises(ValueError, match="scenery"):
        _env(sprites, scenery=True).render_observations()
    with pytest.raises(ValueError, match="render_mode"):
        pikazoo_v0.env(num_envs=4, device=DEV).render_observations()
    env = _env(sprites)
    for scale in (0, 3, 16, 2.5, 2.0, 4.0, True, "4", None):
        with pytest.raises(ValueError, match="scale"):
            env.render_observations(scale)
        with pytest.raises(ValueError, match="scale"):
            PixelObservation(env, scale=scale)
    monkeypatch.setattr(R, "default_image_dir", lambda: None)  # (no installed reference package to find sprites in)
    with pytest.raises(FileNotFoundError):
        pikazoo_v0.env(num_envs=4, device=DEV, render_mode="rgb_array").render_observations()
    monkeypatch.undo()
    big = pikazoo_v0.env(num_envs=1 << 17, device=DEV, render_mode="rgb_array", sprites=sprites, flight_tables=False)
    with pytest.raises(ValueError, match="1 GiB"):
        big.render_observations(1)  # 131 072 x 131 328 bytes
    del big
    good = torch.empty((pj.N, 76, 108), dtype=torch.uint8, device=DEV)
    assert env.render_observations(4, out=good) is good
    wide = torch.empty((pj.N, 76, 216), dtype=torch.uint8, device=DEV)
    flat = torch.empty(pj.N * 76 * 108 + 8, dtype=torch.uint8, device=DEV)
    odd = torch.empty((pj.N, 76 * 108 + 2), dtype=torch.uint8, device=DEV)
    for bad in (torch.empty((pj.N, 76, 108), dtype=torch.int8, device=DEV),            # wrong dtype
                torch.empty((pj.N, 76, 108), dtype=torch.int32, device=DEV),
                torch.empty((pj.N - 1, 76, 108), dtype=torch.uint8, device=DEV),       # wrong frame count
                torch.empty((pj.N, 76, 108, 1), dtype=torch.uint8, device=DEV),        # wrong rank
                torch.empty((pj.N, 38, 54), dtype=torch.uint8, device=DEV),            # another scale's
                torch.empty((pj.N, 76, 108), dtype=torch.uint8),                       # host memory
                wide[:, :, ::2],                                                       # inner dim not contiguous
                wide[:, :, :108],                                                      # rows not contiguous
                flat[2:2 + pj.N * 76 * 108].view(pj.N, 76, 108),                       # pointer not 4-byte aligned
                odd[:, :76 * 108].view(pj.N, 76, 108),                                 # frames 2 bytes off a dword apart
                good.cpu().numpy()):
        with pytest.raises(ValueError, match="out="):
            env.render_observations(4, out=bad)


@pytest.mark.parametrize("kind", ["frame_skip", "mixed", "packed"])
def test_pixel_observation_wrapper(sprites, kind):
    from pikazoo_amd.wrappers import PixelObservation, SimplifyAction

    mask = (np.arange(pj.N) % 3 == 0)
    kw = {"frame_skip": dict(frame_skip=4, is_player2_computer=True), "mixed": dict(is_player2_computer=mask),
          "packed": dict(state_format="packed")}[kind]
    scale = {"frame_skip": 4, "mixed": 8, "packed": 2}[kind]
    h, w = 304 // scale, 432 // scale
    raw = _env(sprites, **kw)
    env = PixelObservation(SimplifyAction(raw), scale=scale)
    assert env.unwrapped is raw
    for agent in (A1, A2):
        space = env.observation_space(agent)
        assert space.shape == (h, w) and space.dtype == np.uint8 and space.low.min() == 0 and space.high.max() == 255
        assert env.action_space(agent).n == 13
    obs, infos = env.reset()
    assert set(obs) == {A1, A2} and obs[A1].shape == (pj.N, h, w) and obs[A1].dtype == torch.uint8
    assert obs[A1].data_ptr() == obs[A2].data_ptr()  # one screen
    assert np.array_equal(obs[A1].cpu().numpy(), pj.frames(raw.read_state().cpu().numpy(), sprites, scale))
    first = obs[A1].data_ptr()
    g = torch.Generator(DEV).manual_seed(2)
    for t in range(25):
        acts = {a: torch.randint(0, 13, (pj.N,), dtype=torch.int32, device=DEV, generator=g) for a in (A1, A2)}
        obs, rew, term, trunc, infos = env.step(acts)
    assert obs[A1].data_ptr() == obs[A2].data_ptr() == first  # allocated once, overwritten
    assert rew[A1].shape == (pj.N,) and term[A1].shape == (pj.N,) and A1 in infos
    want = pj.frames(env.unwrapped.read_state().cpu().numpy(), sprites, scale)
    assert np.array_equal(obs[A1].cpu().numpy(), want), _first_difference(obs[A1].cpu().numpy(), want)
    assert raw.steps_done == 25


def test_scalar_api_returns_a_numpy_screen(sprites):
    from pikazoo_amd import pikazoo_v0
    from pikazoo_amd.wrappers import PixelObservation

    one = pikazoo_v0.env(num_envs=1, scalar_api=True, render_mode="rgb_array", sprites=sprites, seed=2)
    one.reset()
    img = one.render_observations(4)
    assert isinstance(img, np.ndarray) and img.shape == (76, 108) and img.dtype == np.uint8
    assert np.array_equal(img, pj.frames(one.unwrapped.read_state().cpu().numpy(), sprites, 4)[0])
    obs, _ = PixelObservation(one, scale=8).reset()
    assert isinstance(obs[A1], np.ndarray) and obs[A1].shape == (38, 54)


def test_hipgraph_replay_of_the_wrapped_step_equals_eager(sprites):
    from pikazoo_amd.wrappers import PixelObservation

    acts = {a: torch.randint(0, 18, (pj.N,), dtype=torch.int32, device=DEV, generator=torch.Generator(DEV).manual_seed(i))
            for i, a in enumerate((A1, A2))}
    envs = {}
    for mode in ("eager", "graph"):
        env = PixelObservation(_env(sprites, is_player2_computer=True, seed=5), scale=4)
        env.reset()
        env.step(acts)  # (allocates and binds; a capture records launches only)
        envs[mode] = env
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            obs_g = envs["graph"].step(acts)[0]
    side.synchronize()
    for t in range(8):
        with torch.cuda.stream(side):
            graph.replay()
        side.synchronize()
        obs_e = envs["eager"].step(acts)[0]
        assert torch.equal(obs_g[A1], obs_e[A1]), t
    assert torch.equal(envs["graph"].unwrapped.read_state(), envs["eager"].unwrapped.read_state())
    want = pj.frames(envs["eager"].unwrapped.read_state().cpu().numpy(), sprites, 4)
    assert np.array_equal(obs_g[A1].cpu().numpy(), want)
