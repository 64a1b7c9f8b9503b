"""Pixel observations (pz_render_gray) without a GPU: the export, its declaration and binding, argument validation, the
family's census in the code object -- four instantiations outside pz::, none named like the mixed family, no scratch, no
VGPR spill --, that no other kernel's instruction stream moved (tests/golden/kernel_digests_pixel_obs_parent.json: the
digests of the commit before the family), and, on the judge alone, that the GPU cases' planted states bite."""
import ctypes as C
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pixel_judge as pj

REPO = Path(__file__).resolve().parent.parent
KERNELS = {f"pz_pixels::gray_kernel<{s}>" for s in pj.SCALES}


@pytest.fixture(scope="module")
def built_lib():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    sys.path.insert(0, str(REPO / "tools"))
    import build as pz_build

    return pz_build.build()


def test_symbol_is_exported_declared_and_bound(built_lib):
    from pikazoo_amd import _native

    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "pikazoo_hip.h").read_text(), flags=re.S)
    decl = re.search(r"int\s+pz_render_gray\s*\(([^;]*)\)\s*;", header)
    assert decl, "pz_render_gray is not declared in include/pikazoo_hip.h"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert len(params) == 13 and params[8] == "const uint8_t *background_gray" and params[11] == "int64_t frame_stride"
    exported = subprocess.run(["nm", "-D", "--defined-only", str(built_lib)], check=True, capture_output=True, text=True).stdout
    assert re.search(r" T pz_render_gray$", exported, flags=re.M), "pz_render_gray is not exported"
    assert "pz_render_gray" in _native.exported_names()
    lib = _native.load()
    # additive: the ABI version and pz_config are the parent's
    assert lib.pz_abi_version() == _native.ABI_VERSION == 10
    assert lib.pz_config_bytes() == C.sizeof(_native.PzConfig) == 120
    assert len(lib.pz_render_gray.argtypes) == 13
    assert "pz_render_gray" in (REPO / "INTEGRATION.md").read_text()


def test_argument_validation_without_a_gpu(built_lib):
    from pikazoo_amd import _native

    lib = _native.load()
    fake = C.c_void_p(4096)  # never dereferenced: every call below returns before a launch

    def call(state=fake, n=8, stride=8, lanes=None, m=0, atlas=fake, sprites=fake, background=fake, gray=None, scale=4,
             frames=fake, frame_stride=76 * 108):
        return lib.pz_render_gray(state, n, stride, lanes, m, atlas, sprites, background, gray, scale, frames, frame_stride, None)

    assert call() == 0                                            # m == 0: no launch
    assert call(gray=fake) == 0 and call(lanes=fake) == 0
    for scale, size in ((1, 304 * 432), (2, 152 * 216), (4, 76 * 108), (8, 38 * 54)):
        assert call(scale=scale, frame_stride=size) == 0
        assert call(scale=scale, frame_stride=size - 4) == -2     # frames would overlap
        assert call(scale=scale, frame_stride=3 * size) == 0      # slot of a frame stack
    for name in ("state", "atlas", "sprites", "background", "frames"):
        assert call(**{name: None}) == -1, name
    for scale in (0, 3, 5, 16, -1):
        assert call(scale=scale) == -3, scale
    assert call(frames=C.c_void_p(4098)) == -4 and call(frames=C.c_void_p(4097)) == -4
    assert call(frame_stride=76 * 108 + 2) == -4
    assert call(gray=C.c_void_p(4098)) == -4                      # looked up a dword at a time
    assert call(n=8, stride=4) == -2 and call(n=-1) == -2 and call(m=-1) == -2
    assert call(m=9) == -2                                        # lanes == NULL: games 0..m-1, m <= n


def test_the_code_object_holds_exactly_the_four_instantiations_outside_pz(built_lib):
    import kernel_digest
    import kernel_notes

    if not kernel_digest.available():
        pytest.skip("llvm-objdump not available")
    names = set(kernel_digest.kernels(built_lib))
    assert {n for n in names if not n.startswith(("pz::", "pz_mixed::"))} == KERNELS
    assert not any("mixed" in n for n in KERNELS)
    assert {n for n in names if "gray" in n or "pixel" in n} == KERNELS  # nothing of the family inside pz::
    rows = {name.split("(")[0].replace("void ", ""): r for name, r in kernel_notes.notes(Path(built_lib))}
    for k in KERNELS:
        r = rows[k]
        assert r[".private_segment_fixed_size"] == 0, f"{k} uses scratch memory"
        assert r[".vgpr_spill_count"] == 0, f"{k} spills VGPRs"
        assert r[".group_segment_fixed_size"] == 12 * 32  # the resolved draw list, nothing else


def test_no_other_kernel_moved(built_lib):
    """render_kernel, every step / rollout / hold kernel and everything else the parent commit shipped carry the parent's
    instruction-stream digest (tools/kernel_digest.py): the family was added beside them."""
    import kernel_digest

    if not kernel_digest.available():
        pytest.skip("llvm-objdump not available")
    parent = json.loads((REPO / "tests" / "golden" / "kernel_digests_pixel_obs_parent.json").read_text())
    assert "pz::render_kernel" in parent and sum(n.startswith("pz::step_") for n in parent) > 50
    now = {n: d for n, (d, _) in kernel_digest.kernels(built_lib).items()}
    assert set(now) - KERNELS == set(parent)
    moved = sorted(n for n in parent if now[n] != parent[n])
    assert not moved, moved


@pytest.fixture(scope="module")
def sprite_set():
    from pikazoo_amd.render import synthetic_sprites

    return synthetic_sprites(7, "cpu")


def test_the_judge_is_the_frame_oracle_and_the_product_reduction(sprite_set):
    from oracle import render_oracle as ro
    from pikazoo_amd.render import SPRITE_SHAPES, gray_downsample

    assert pj.SPRITE_SIZES == SPRITE_SHAPES
    st = pj.states()
    assert st.shape == (44, pj.N) and pj.N == 64 + 6
    for lane in (pj.POWER, pj.SCORES, pj.WALL_LEFT, 40):
        full = ro.frame(st[:, lane], sprite_set.sprites_host, sprite_set.background_host)
        assert np.array_equal(pj.compose(st[:, lane], sprite_set.sprites_host, sprite_set.background_host), full)
        for scale in pj.SCALES:  # the host's background reduction (the kernel's fast path) is the judge's
            assert np.array_equal(gray_downsample(full, scale), pj.gray_downsample(full, scale))
    # by hand: a frame of one colour, and one bright pixel in a block
    flat = np.zeros((304, 432, 3), np.uint8) + np.array([10, 200, 30], np.uint8)
    y = (77 * 10 + 150 * 200 + 29 * 30 + 128) >> 8
    for scale in pj.SCALES:
        out = pj.gray_downsample(flat, scale)
        assert out.shape == (304 // scale, 432 // scale) and (out == y).all()
    flat[8, 16] = 255
    assert pj.gray_downsample(flat, 8)[1, 2] == (63 * y + 255 + 32) >> 6 and pj.gray_downsample(flat, 1)[8, 16] == 255


def test_the_planted_states_hold_the_situations_the_gpu_cases_name():
    from oracle import render_oracle as ro

    st = pj.states()
    P2 = ro.P_WORDS
    assert st[ro.B_POWER, pj.POWER] == 1 and st[ro.B_POWER, pj.BALL_TOP] == 1
    assert st[ro.P_STATE, pj.DIVE_P1] == 3 and st[ro.P_DIVE, pj.DIVE_P1] == -1            # mirrored
    assert st[P2 + ro.P_STATE, pj.DIVE_P2] == 3 and st[P2 + ro.P_DIVE, pj.DIVE_P2] == 1   # the one unmirrored player 2
    assert st[ro.E_S1, pj.SCORES] >= 10 and st[ro.E_S2, pj.SCORES] >= 10
    assert st[ro.B_Y, pj.BALL_TOP] < 20 and st[ro.B_X, pj.BALL_LEFT] < 20 and st[ro.B_X, pj.BALL_RIGHT] > 412
    assert st[ro.B_Y, pj.BALL_BOTTOM] > 304 - 20
    assert st[ro.P_X, pj.WALL_LEFT] < 32 and pj.diving(st[:, pj.WALL_LEFT], 0)
    assert st[P2 + ro.P_X, pj.WALL_RIGHT] > 432 - 32 and pj.diving(st[:, pj.WALL_RIGHT], 1)


@pytest.fixture(scope="module")
def planted_frames(sprite_set):
    st = pj.states()
    full = [pj.compose(st[:, l], sprite_set.sprites_host, sprite_set.background_host) for l in range(pj.N)]
    return st, full


@pytest.mark.parametrize("scale", pj.SCALES)
def test_every_slot_of_the_draw_list_shows_in_some_lane(sprite_set, planted_frames, scale):
    """Non-vacuity, on the judge alone: leaving out any one of the twelve slots changes at least one output byte of some
    planted lane at this scale -- a kernel that skipped the slot is caught."""
    st, full = planted_frames
    for slot in range(pj.SLOTS):
        lanes = [l for l in range(pj.N) if slot in pj.drawn_slots(st[:, l])]
        assert lanes, slot
        assert any(not np.array_equal(
            pj.gray_downsample(pj.compose(st[:, l], sprite_set.sprites_host, sprite_set.background_host, drop=slot), scale),
            pj.gray_downsample(full[l], scale)) for l in lanes), (slot, scale)


@pytest.mark.parametrize("scale", pj.SCALES)
def test_mirroring_a_diving_player_shows(sprite_set, planted_frames, scale):
    st, full = planted_frames
    for p, lane in ((0, pj.DIVE_P1), (1, pj.DIVE_P2), (0, pj.WALL_LEFT), (1, pj.WALL_RIGHT)):
        assert pj.diving(st[:, lane], p)
        other = pj.compose(st[:, lane], sprite_set.sprites_host, sprite_set.background_host, mirror=p)
        assert not np.array_equal(pj.gray_downsample(other, scale), pj.gray_downsample(full[lane], scale)), (p, lane, scale)


def test_the_lone_shadow_shows_at_scale_8(sprite_set, planted_frames):
    """The 32 x 8 shadow is the smallest blit: in the lane planted for it, where nothing else is drawn near, leaving the
    ball's shadow out changes the scale-8 frame."""
    st, full = planted_frames
    lane = pj.SHADOW_ALONE
    without = pj.compose(st[:, lane], sprite_set.sprites_host, sprite_set.background_host, drop=5)
    a, b = pj.gray_downsample(without, 8), pj.gray_downsample(full[lane], 8)
    rows, cols = np.nonzero(a != b)
    assert rows.size and set(rows) <= {33, 34} and cols.min() >= 200 // 8 and cols.max() <= 232 // 8
