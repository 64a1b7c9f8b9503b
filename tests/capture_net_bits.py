#!/usr/bin/env python3
"""tests/golden/net_forward_bits.json: digests of what ``pz_mlp_forward`` WROTE on seeded inputs (GPU machine only).

    python tests/capture_net_bits.py

Every other test of the net allows a tolerance; this record pins the bits, so that a change meant to leave the kernels'
arithmetic alone can be held to exactly that.  It was taken from the library of the commit BEFORE the two forward
libraries came to share csrc/pz_mlp_tile.hpp, and is never regenerated from the code it judges.  Stored: the library's
build id, the compiler's version line, and per case a SHA-256 of the input bytes (a changed ``net_judge.make_obs`` /
``make_params`` then reads as "inputs differ", not "kernel moved") and one of each agent's ``[n, O]`` output elements
(pads excluded; a 16-bit output as the float32 values it stands for).  tests/test_gpu_net.py holds the library to it.
"""
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "pika-zoo_amd"):  # (tests/conftest.py does the same under pytest)
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import net_judge as N  # noqa: E402

PATH = REPO / "tests" / "golden" / "net_forward_bits.json"
SIZES = ((35, 64, 19), (35, 32, 19), (35, 128, 19), (1, 32, 1), (36, 64, 33), (72, 128, 40))


def cases():
    """(name, [obs per agent], obs format, [parameter set per agent], activation, output format)"""
    def pair(n, K, H, O, obs_dtype="float32"):  # two agents with nets of their own: test_batch_sizes' seeds
        return [N.make_obs(n, K, obs_dtype, seed) for seed in (3, 4)], [N.make_params(K, H, O, seed) for seed in (1, 2)]

    for K, H, O in SIZES:
        for activation in N.ACTIVATIONS:
            obs, params = pair(129, K, H, O)
            yield f"{K}-{H}-{O} {activation} n=129", obs, "float32", params, activation, "float32"
    K, H, O = SIZES[0]
    for obs_dtype in N.OBS_DTYPES:
        for out_dtype in N.OUT_DTYPES:
            obs, params = pair(129, K, H, O, obs_dtype)
            yield f"{obs_dtype} -> {out_dtype} n=129", obs, obs_dtype, params, "tanh", out_dtype
    # 40 000 rows: with two agents the grid is capped at half the resident workgroups, so some waves take a second tile
    for n in (1, 33, 4099, 40000):
        obs, params = pair(n, K, H, O)
        yield f"n={n}", obs, "float32", params, "tanh", "float32"
    for activation in N.ACTIVATIONS:  # test_nan_containment's inputs
        obs = N.make_obs(70, K, "float32", 14)
        obs[5, 17] = np.nan
        obs[40, 0] = np.inf
        obs[69, K - 1] = np.nan
        yield f"nan containment {activation}", [obs], "float32", [N.make_params(K, H, O, 13)], activation, "float32"
    # test_int32_beyond_2_to_24_rounds_to_nearest_even's inputs
    obs = np.array([[2 ** 24 + 1, -(2 ** 24 + 3), 2 ** 30 + 65, 7]] * 3, np.int32)
    params = N.make_params(4, 32, 3, 12)
    params[0] = (params[0] * np.float32(2.0 ** -30)).astype(np.float32)
    yield "int32 beyond 2^24", [obs], "int32", [params], "tanh", "float32"


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digests(lib, run_forward, obs_bits):
    """{case: {"inputs": digest, "outputs": [digest per agent]}} of the loaded library (`run_forward`, `obs_bits`:
    tests/test_gpu_net.py's, which also checks every buffer for what must not have been written)"""
    out = {}
    for name, obs, obs_dtype, params, activation, out_dtype in cases():
        have = run_forward(lib, obs, obs_dtype, params, activation, out_dtype)
        out[name] = {"inputs": sha([obs_bits(x, obs_dtype) for x in obs] + [np.asarray(p, np.float32) for ps in params for p in ps]),
                     "outputs": [sha([y.astype(np.float32).view(np.uint32)]) for y in have]}
    return out


def compiler_line():
    """the line of ``hipcc --version`` that names the compiler (tanhf comes from the toolchain)"""
    from pikazoo_amd import _native

    text = subprocess.run([_native._pz_build().hipcc_path(), "--version"], capture_output=True, text=True, check=True).stdout
    return next(line for line in text.splitlines() if "clang version" in line).strip()


if __name__ == "__main__":
    from pikazoo_amd import net

    import test_gpu_net as T

    lib = net.load()
    record = {"build_id": lib.pz_net_build_id().decode(), "compiler": compiler_line(), "cases": digests(lib, T.run_forward, T.obs_bits)}
    PATH.write_text(json.dumps(record, indent=1) + "\n")
    print(PATH, PATH.stat().st_size, "bytes,", len(record["cases"]), "cases, build id", record["build_id"])
