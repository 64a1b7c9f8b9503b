"""The C++ kernel choice against its spec, on the host (no GPU): pika-zoo_amd/csrc/pz_dispatch.hpp, compiled with the host
compiler behind tests/dispatch_shim.cpp, names the instantiation tests/kernel_matrix.py `dispatch()` names -- over the
whole input space of the choice and for every configuration of tests/kernel_configs.py -- and its image, the
instantiations the library builds, is exactly the kernel matrix.  (tests/test_gpu_kernel_matrix.py checks the kernel
a launch really ran, by name, on the GPU.)"""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import pytest

import kernel_configs as kc
import kernel_matrix as km
from pikazoo_amd import _native

REPO = Path(__file__).resolve().parent.parent

# the four states of the flight tables -> (the power-hit table is passed, kernel_matrix's table mode): the landing table
# alone dispatches like no tables
TABLES = {"both": (True, "both"), "power_hit": (True, "power_hit"), "landing": (False, "none"), "none": (False, "none")}
# every way a configuration is PLAIN or fused: (pz_config words, a statistics pointer is passed)
FORMS = (({}, False), ({}, True), ({"simplify_action": 1}, False), ({"ballpos_reward": 1}, False),
         ({"normal_state_mode": 1}, False), ({"normal_state_mode": 2}, False), ({"episode_stats_mode": 1}, True),
         ({"episode_stats_mode": 2}, True), ({"episode_stats_mode": 1}, False), ({"episode_stats_mode": 2}, False))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("dispatch") / "dispatch_shim.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", f"-I{REPO / 'include'}",
                           f"-I{REPO / 'pika-zoo_amd' / 'csrc'}", "-o", str(so), str(REPO / "tests" / "dispatch_shim.cpp")])
    lib = C.CDLL(str(so))
    lib.pz_test_choose.argtypes = [C.c_int, C.c_int, C.c_int64, C.POINTER(_native.PzConfig), C.c_int, C.c_int, C.c_char_p,
                                   C.c_int]
    lib.pz_test_choose.restype = None
    lib.pz_test_image.argtypes = [C.c_int, C.c_char_p, C.c_int]
    return lib


def choose(shim, entry, k, n, fields, stats, power_hit) -> str:
    cfg = _native.PzConfig(**fields)
    name = C.create_string_buffer(128)
    shim.pz_test_choose(km._MODE[entry], k, n, C.byref(cfg), int(stats), int(power_hit), name, len(name))
    return name.value.decode()


def test_the_choice_is_the_spec_over_its_whole_input_space(shim):
    """entry point x k x n on both sides of the switch x state format x all seven row formats x every PLAIN / fused factor
    (a statistics mode without a pointer included) x four table states x player mix"""
    sizes = (km.N_BELOW, km.SWITCH - 1, km.SWITCH, km.N_ABOVE)
    seen = set()
    for entry, k, n, packed, fmt, (form, stats), tables, (p1, p2) in itertools.product(
            km._MODE, (1, 5), sizes, (0, 1), range(7), FORMS, TABLES, km.MIXES):
        fields = kc.config_fields(p1_computer=p1, p2_computer=p2, packed_state=packed, normalize_obs=fmt, **form)
        power_hit, spec_tables = TABLES[tables]
        want = km.dispatch(entry, k, n, fields, stats, spec_tables)
        assert choose(shim, entry, k, n, fields, stats, power_hit) == want, (entry, k, n, fields, stats, tables)
        seen.add(want)
    assert seen == km.KERNELS


def test_every_runtime_configuration_reaches_its_instantiation_through_the_choice(shim):
    configs = kc.configs()
    assert configs
    for c in configs:
        want = km.dispatch(c.entry, c.k, c.n, c.fields(), c.stats_ptr, c.tables)
        assert choose(shim, c.entry, c.k, c.n, c.fields(), c.stats_ptr, c.tables != "none") == want == c.kernel, c.name


def test_the_instantiations_are_the_image_of_the_choice(shim):
    """step_kernel_image(): what the product library instantiates (tests/test_cabi_and_host.py compares the matrix with
    the library's code object)"""
    name = C.create_string_buffer(128)
    count = shim.pz_test_image(0, name, len(name))
    image = []
    for i in range(count):
        shim.pz_test_image(i, name, len(name))
        image.append(name.value.decode())
    assert len(image) == len(set(image)) == len(km.KERNELS)
    assert set(image) == km.KERNELS
