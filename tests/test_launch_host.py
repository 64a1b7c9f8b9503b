"""CPU tests (no GPU needed) of ``pikazoo_amd._launch``, the plumbing that the learner's nine bindings share: the error path
of a launch in a module's own words, that importing it imports no binding and loads no library, that ``batch``, ``optim`` and
``league`` no longer import ``net``, and that every shared helper is defined in one file of the package only."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
PACKAGE = REPO / "pika-zoo_amd" / "pikazoo_amd"
BINDINGS = ("learn", "policy", "ppo", "net", "netgrad", "optim", "batch", "pool", "league")


def child(code):
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); " + code, str(REPO / "pika-zoo_amd")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_check_speaks_in_the_words_of_the_module_it_is_given():
    from pikazoo_amd import _launch, _native, batch, net

    assert _launch.check(0, "pz_mlp_forward", net._ERRORS) is None
    for code, text in ((-1, "a required pointer is NULL"), (-2, "a size or a pitch beyond the kernel's range"),
                       (-4, "a pointer not aligned to its element"), (1, "HIP error")):
        with pytest.raises(_native.PikazooNativeError) as e:
            _launch.check(code, "pz_mlp_forward", net._ERRORS)
        assert str(e.value) == f"pz_mlp_forward failed: {text} (code {code})"
    # a module's table holds the two shared texts and its own; batch alone words -4 for itself
    for name in BINDINGS:
        table = getattr(__import__(f"pikazoo_amd.{name}", fromlist=[name]), "_ERRORS")
        assert sorted(table) == [-4, -3, -2, -1] and table[-1] == _launch.ERRORS[-1], name
        assert table[-4] == (_launch.ERRORS[-4] if name != "batch" else "a pointer, pitch or row not aligned to its element"), name
    with pytest.raises(_native.PikazooNativeError) as e:
        _launch.check(-4, "pz_batch_copy", batch._ERRORS)
    assert str(e.value) == "pz_batch_copy failed: a pointer, pitch or row not aligned to its element (code -4)"


def test_importing_the_plumbing_imports_no_binding_and_loads_no_library():
    child("import pikazoo_amd._launch; "
          f"assert not [m for m in {BINDINGS!r} if 'pikazoo_amd.' + m in sys.modules]; "
          "assert not any('libpikazoo' in line for line in open('/proc/self/maps')); print('ok')")


@pytest.mark.parametrize("name", ["batch", "optim", "league"])
def test_these_bindings_no_longer_import_the_net_module(name):
    child(f"from pikazoo_amd import {name}; assert 'pikazoo_amd.net' not in sys.modules; "
          "assert not any('libpikazoo' in line for line in open('/proc/self/maps')); print('ok')")


def test_every_shared_helper_is_defined_in_one_file():
    sources = {p.name: p.read_text() for p in sorted(PACKAGE.glob("*.py"))}
    # the old names and the new ones: a definition of either, in any file but _launch.py, is a copy
    helpers = {"span": ("_span",), "no_alias": ("_no_alias",), "sides": ("_sides",), "shape": ("_shape",), "ptrs": ("_ptrs",),
               "raw_stream": ("_stream", "_raw_stream"), "check": ("_check", "_fail"), "describe": ("_describe",),
               "device_index": ("_index",), "check_workspace": ("_check_workspace",), "launch": ()}
    for new, old in helpers.items():
        pattern = re.compile(r"^def (?:%s)\(" % "|".join((new, *old)), re.M)  # (module level: env has a method _stream)
        where = [name for name, text in sources.items() if pattern.search(text)]
        if new == "check":  # (_native.check is the product library's own: it asks the library for the text)
            where.remove("_native.py")
        assert where == ["_launch.py"], (new, where)
    assert [name for name, text in sources.items() if "_cuda_getCurrentRawStream" in text] == ["_launch.py"]
    # ... and none of the sentences is written out a second time
    for sentence in ("overlaps {other}: outputs must not alias", "{what}: a dict of one or two agents", "the workspace must be", "failed: {",
                     "dev.index if dev.index is not None"):
        where = [name for name, text in sources.items() if sentence in text]
        assert where in (["_launch.py"], ["_launch.py", "_native.py"]), (sentence, where)
    # the MLP argument check stands in net.py alone
    for sentence in ("obs must have shape [N, K]", "hidden must be one of", "{label.format(m)}{name} must be a contiguous float32", "out_dtype must be"):
        where = [name for name, text in sources.items() if sentence in text]
        assert where == ["net.py"], (sentence, where)
