"""CPU tests (no GPU needed) of the float16 / bfloat16 observation formats (include/pikazoo_hip.h enum pz_obs_format,
3 - 6): the C ABI accepts them and applies the 2-byte row rules before any launch, and the product code object rounds to
nearest even (no round-toward-zero conversion anywhere)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
FLOAT16_FORMATS = (3, 4, 5, 6)  # float16, bfloat16, float16 normalized, bfloat16 normalized


@pytest.fixture(scope="module")
def built_lib():
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build as pz_build

    return pz_build.build()


@pytest.fixture(scope="module")
def lib(built_lib):
    from pikazoo_amd import _native

    return _native.load()


def _cfg(fmt):
    from pikazoo_amd import _native

    cfg = _native.PzConfig()
    cfg.winning_score, cfg.serve_mode, cfg.normalize_obs = 15, 0, fmt
    return cfg


def test_the_float16_formats_pass_argument_validation(lib):
    """Empty-batch calls return before a launch: 0 for the formats 0 - 6, PZ_E_CONFIG for anything else."""
    fake = C.c_void_p(4096)  # never dereferenced: every call below returns before a launch
    for fmt in (0, 1, 2) + FLOAT16_FORMATS:
        cfg = _cfg(fmt)
        assert lib.pz_init(fake, 0, 0, C.byref(cfg), None) == 0, fmt
        assert lib.pz_reset(fake, 0, 0, C.byref(cfg), None, fake, fake, None, None) == 0, fmt
        assert lib.pz_step(fake, 0, 0, C.byref(cfg), fake, fake, fake, fake, fake, fake, fake, None, None, None) == 0, fmt
        assert lib.pz_observe(fake, 0, 0, fmt, 0, fake, fake, None) == 0, fmt
        assert lib.pz_observe(fake, 0, 0, fmt, 1, fake, fake, None) == 0, fmt
    for fmt in (7, -1, 1 << 20):
        cfg = _cfg(fmt)
        assert lib.pz_init(fake, 0, 0, C.byref(cfg), None) == -3, fmt                      # PZ_E_CONFIG
        assert lib.pz_step(fake, 0, 0, C.byref(cfg), fake, fake, fake, fake, fake, fake, fake, None, None, None) == -3
        assert lib.pz_observe(fake, 0, 0, fmt, 0, fake, fake, None) == -3, fmt


def test_k_frame_launches_need_n_divisible_by_8_on_every_2_byte_format(lib):
    """A [n][35] frame of 2-byte rows keeps the 16-byte alignment of the vector stores only for n % 8 == 0 (70 * n % 16):
    n = 4100 is refused with PZ_E_ALIGN before a launch for every 2-byte format."""
    fake = C.c_void_p(4096)
    n = 4100
    assert n % 4 == 0 and n % 8 != 0
    for fmt in (2,) + FLOAT16_FORMATS:
        cfg = _cfg(fmt)
        assert lib.pz_rollout_random(fake, n, n, C.byref(cfg), 1, 0, 2, None, fake, fake, fake, fake, fake, None, None,
                                     None, None) == -4, fmt
        assert lib.pz_step_many(fake, n, n, C.byref(cfg), fake, 2, fake, fake, fake, fake, fake, None, None, None,
                                None) == -4, fmt
    # a single frame takes any row count (an odd one is padded by a row): the empty batch returns before a launch
    for fmt in (2,) + FLOAT16_FORMATS:
        cfg = _cfg(fmt)
        assert lib.pz_rollout_random(fake, 0, 0, C.byref(cfg), 1, 0, 1, None, fake, fake, fake, fake, fake, None, None,
                                     None, None) == 0, fmt


def test_no_round_toward_zero_conversion_in_the_product():
    """float16 / bfloat16 rows are the round-to-nearest-even conversion of the float32 value: the code object holds
    the RNE conversions and never v_cvt_pkrtz_f16_f32 (round toward zero)."""
    sys.path.insert(0, str(REPO / "pika-zoo_amd"))
    import build as pz_build

    built = pz_build.build()
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not available")
    import tempfile

    with tempfile.TemporaryDirectory() as t:
        copy = shutil.copy(built, Path(t) / "lib.so")
        subprocess.run([objdump, "--offloading", str(copy)], check=True, cwd=t, capture_output=True)
        objs = [p for p in Path(t).iterdir() if "gfx950" in p.name]
        assert objs, "no gfx950 code object"
        asm = subprocess.run([objdump, "-d", str(objs[0])], check=True, capture_output=True, text=True).stdout
    mnemonics = re.findall(r"^\s+(v_cvt_[a-z0-9_]+)", asm, flags=re.M)
    assert "v_cvt_f16_f32_e32" in mnemonics or "v_cvt_f16_f32_e64" in mnemonics, "no float16 conversion found"
    assert "v_cvt_pk_bf16_f32" in mnemonics, "no bfloat16 conversion found"
    assert not any("pkrtz" in m for m in mnemonics), "a round-toward-zero float16 conversion is in the product"
