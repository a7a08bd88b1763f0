"""tools/abkit.py on the CPU: the variant grammar, Variant.applied and _lib.use put everything back, interleave's statistics.  The
planner options live in the host code of libstep_amd.so, so no device is needed (the library is taken as tests/test_planner.py takes it)."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import pytest

from step_amd import _capi, _lib, backbone, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "step_amd", "libstep_amd.so")

spec = importlib.util.spec_from_file_location("abkit", os.path.join(ROOT, "tools", "abkit.py"))
abkit = importlib.util.module_from_spec(spec)
spec.loader.exec_module(abkit)
V = abkit.Variant.parse


@pytest.fixture
def lib():
    """the product library as _lib.lib(), every option at its default before and after"""
    if not os.path.exists(LIB):
        pytest.skip("libstep_amd.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    L = _capi.declare(ctypes.CDLL(LIB))
    L.step_reset_options()
    with _lib.use(L):
        yield L
    L.step_reset_options()


def options(L):
    return {k: _capi.get_option(L, k) for k in _capi.OPTION_IDS}


def test_grammar():
    for text in ("default", "", None, ",default,"):
        v = V(text)
        assert (v.lib, v.options, v.switches) == (None, {}, ())
    v = V("conv_persist=0,lib=prev,conv_nb_rule=1,backbone.FUSE_CONV_POOL=False,ops.POOL_CONV_MAX_NB=3")
    assert v.lib == "prev" and v.options == {"conv_persist": 0, "conv_nb_rule": 1}
    assert v.switches == (("backbone", "FUSE_CONV_POOL", False), ("ops", "POOL_CONV_MAX_NB", 3))
    assert type(v.switches[0][2]) is bool and type(v.switches[1][2]) is int
    # the three spellings of the first flag_ab.py: bb. for backbone., ops. as it is, opt: in front of a planner option; a bool written 0 / 1
    assert V("bb.FUSE_CONV_POOL=0") == V("backbone.FUSE_CONV_POOL=False")
    assert type(V("bb.POOL_WITH_POINTWISE=1").switches[0][2]) is bool
    assert V("ops.POOL_CONV_MAX_NB=3").switches == (("ops", "POOL_CONV_MAX_NB", 3),)
    assert V("opt:conv_tail=0") == V("conv_tail=0")
    assert ops.PROFILE is None and V("ops.PROFILE=3").switches == (("ops", "PROFILE", 3),)      # an attribute that holds None takes any literal
    assert V("bb.FUSE_CONV_POOL=0,opt:conv_tail=0,lib=x") == V("lib=x,conv_tail=0,backbone.FUSE_CONV_POOL=False")


@pytest.mark.parametrize("text", ["conv_nosuch=1", "opt:conv_nosuch=1", "conv_tail=0,backbone.NO_SUCH_SWITCH=1", "nosuchmodule.X=1",
                                  "backbone.FUSE_CONV_POOL=3", "backbone.FUSE_CONV_POOL='no'", "ops.POOL_CONV_MAX_NB=True",
                                  "ops.POOL_CONV_MAX_NB=2.0", "ops.POOL_CONV_MAX_NB=open", "lib=a,conv_tail=0,lib=b", "conv_tail", "conv_tail=x"])
def test_refused_at_parse_time_with_nothing_set(lib, text):
    before, fuse, nb = options(lib), backbone.FUSE_CONV_POOL, ops.POOL_CONV_MAX_NB
    with pytest.raises(ValueError):
        V(text)
    assert options(lib) == before and backbone.FUSE_CONV_POOL is fuse and ops.POOL_CONV_MAX_NB is nb


@pytest.mark.parametrize("fail", [False, True])
def test_applied_sets_and_restores(lib, fail):
    defaults, fuse, nb = options(lib), backbone.FUSE_CONV_POOL, ops.POOL_CONV_MAX_NB
    v = V("conv_waves=4,conv_nb_rule=1,backbone.FUSE_CONV_POOL=False,ops.POOL_CONV_MAX_NB=3")
    try:
        with v.applied() as L:
            assert L is lib and _lib.lib() is lib
            assert _capi.get_option(lib, "conv_waves") == 4 and _capi.get_option(lib, "conv_nb_rule") == 1
            assert {k: x for k, x in options(lib).items() if k not in v.options} == {k: x for k, x in defaults.items() if k not in v.options}
            assert backbone.FUSE_CONV_POOL is False and ops.POOL_CONV_MAX_NB == 3
            if fail:
                raise KeyError("inside")
    except KeyError:
        assert fail
    assert options(lib) == defaults
    assert backbone.FUSE_CONV_POOL is fuse and ops.POOL_CONV_MAX_NB is nb and type(fuse) is bool and type(nb) is int
    assert _lib.lib() is lib


def test_applied_starts_from_defaults_and_returns_to_what_was_set(lib):
    defaults = options(lib)
    _capi.set_option(lib, "conv_tail", 0)
    _capi.set_option(lib, "conv_nb_rule", 1)
    before = options(lib)
    assert before != defaults
    with V("conv_nb_rule=0,conv_waves=4").applied():
        assert _capi.get_option(lib, "conv_tail") == defaults["conv_tail"]            # reset per variant: nothing leaks in
        assert _capi.get_option(lib, "conv_nb_rule") == 0 and _capi.get_option(lib, "conv_waves") == 4
    assert options(lib) == before                                                   # ... and the caller's own settings come back


def test_missing_build_names_the_recipe():
    with pytest.raises(FileNotFoundError, match="build_prev.sh.*EXP="):
        abkit.load_build("no_such_build")
    with pytest.raises(FileNotFoundError):
        with V("lib=no_such_build").applied():
            pass


def test_lib_use_nests_and_restores():
    a, b, start = object(), object(), _lib._LIB
    with _lib.use(a):
        assert _lib.lib() is a
        with _lib.use(b):
            assert _lib.lib() is b
        assert _lib.lib() is a
        with pytest.raises(KeyError):
            with _lib.use(b):
                with _lib.use(a):
                    raise KeyError("two deep")
        assert _lib.lib() is a
    assert _lib._LIB is start


@pytest.mark.parametrize("rounds", [3, 4, 5])
def test_interleave_statistics(rounds):
    script = {("A", "one"): [5.0, 1.0, 4.0, 2.0, 3.0], ("A", "two"): [0.5, 0.4, 0.3, 0.2, 0.1],
              ("B", "one"): [9.0, 8.0, 7.0, 6.0, 5.5], ("B", "two"): [2.0, 2.0, 1.0, 3.0, 0.7]}
    calls = []

    def leg(name):
        def run(v):
            calls.append((v, name))
            return script[v, name][sum(1 for c in calls if c == (v, name)) - 1]
        return run
    res = abkit.interleave(["A", "B"], {"one": leg("one"), "two": leg("two")}, rounds)
    assert calls == [("A", "one"), ("A", "two"), ("B", "one"), ("B", "two")] * rounds       # variants alternate inside every round
    for r, v in zip(res, "AB"):
        for name in ("one", "two"):
            want = sorted(script[v, name][:rounds])
            assert list(r[name]) == want and r[name].median == want[rounds // 2] and r[name].min == min(want)
    same = abkit.interleave(["A", "A"], {"one": lambda v: 1.0}, rounds)                      # equal variants stay apart
    assert [len(r["one"]) for r in same] == [rounds, rounds]


@pytest.mark.parametrize("tool", ["step_ab.py", "flag_ab.py", "two_in_flight.py", "bench_with.py"])
def test_help_needs_no_device(tool):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert p.returncode == 0 and "usage" in p.stdout, p.stderr[-600:]
