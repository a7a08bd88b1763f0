"""tools/abkit.py -- the ONE measuring kit of tools/: experiment builds, variants, the captured-step A/B loop, timers, the report tee.

Boxes of the pool differ by 5-10 %, so only variants interleaved in ONE process are compared; what such a run fixes is decided here, once:

  * streams: bench.py's arrangement -- batch 0 on the default stream, every further batch on a side stream of its own (`streams`);
  * capture: two eager calls per batch, then one HIP graph per batch (`capture_step`);
  * replay: 20 warm replays of batch 0, then `steps` replays round-robin over the batches in flight, host clock, one synchronise (`replay_ms`);
  * statistics: per variant and leg the SORTED per-round times; the median is element len // 2, the minimum element 0 (`Times`);
  * a variant starts from the library's default options and leaves everything as it found it (`Variant.applied`).

A variant is a comma list of
    default | (empty)                      nothing: the working tree's library, default options
    lib=NAME                               tools/libstep_amd_NAME.so (`load_build`), at most one
    conv_persist=0                         a planner option (step_set_option; names: _capi.OPTION_IDS)
    backbone.FUSE_CONV_POOL=False          a module switch of step_amd: a Python literal of the attribute's own type (an int for a float is
                                           taken, anything for an attribute that holds None; no literal with a comma in it: items split there)
`bb.X=..`, `ops.X=..` and `opt:name=..` are the spellings of the first tools/flag_ab.py (it wrote a bool switch as 0 / 1); they parse to the same.
"""
import argparse
import ast
import contextlib
import ctypes
import importlib
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from step_amd import _capi, _lib  # noqa: E402

_BUILDS = {}
_MODULE_ALIASES = {"bb": "backbone"}


def load_build(name, strict=False):
    """the declared handle of tools/libstep_amd_<name>.so: `prev` from tools/build_prev.sh, `probe` from `make -C step_amd/csrc PROBE=1`,
    experiment builds from `make -C step_amd/csrc EXP=<name> EXPFLAGS=-D...`.  Older builds may lack symbols, hence strict=False;
    strict=True raises at once when the build lacks a symbol of include/step_amd.h (a stale probe build)"""
    if strict:
        return _capi.declare(load_build(name))
    if name not in _BUILDS:
        path = os.path.join(HERE, "libstep_amd_%s.so" % name)
        if not os.path.exists(path):
            raise FileNotFoundError("%s not found: tools/build_prev.sh builds `prev`, `make -C step_amd/csrc EXP=%s EXPFLAGS=-D...` an experiment "
                                    "build, `make -C step_amd/csrc PROBE=1` the probe build" % (path, name))
        _BUILDS[name] = _capi.declare(ctypes.CDLL(path), strict=False)
    return _BUILDS[name]


def _options_of(L):
    """{name: value} of every planner option `L` knows (an older build knows fewer)"""
    out = {}
    for name, k in _capi.OPTION_IDS.items():
        v = ctypes.c_int()
        if L.step_get_option(k, ctypes.byref(v)) == 0:
            out[name] = v.value
    return out


class Variant:
    """one parsed variant: .lib (NAME or None), .options {name: int}, .switches ((module, attribute, value), ...), .text as given"""

    def __init__(self, text, lib, options, switches):
        self.text, self.lib, self.options, self.switches = text, lib, options, switches

    def __eq__(self, other):
        return (self.lib, self.options, self.switches) == (other.lib, other.options, other.switches)

    def __repr__(self):
        return "Variant(lib=%r, options=%r, switches=%r)" % (self.lib, self.options, self.switches)

    @classmethod
    def parse(cls, text):
        """validates everything and sets nothing; ValueError names the offending item"""
        lib, options, switches = None, {}, []
        for item in (s.strip() for s in (text or "").split(",")):
            if item in ("", "default"):
                continue
            key, eq, val = item.partition("=")
            if not eq:
                raise ValueError("variant item %r: expected name=value" % item)
            if key == "lib":
                if lib is not None:
                    raise ValueError("variant %r: more than one lib=" % text)
                lib = val
            elif "." in key:
                mod, attr = key.rsplit(".", 1)
                mod = _MODULE_ALIASES.get(mod, mod)
                try:
                    m = importlib.import_module("step_amd." + mod)
                except ImportError:
                    raise ValueError("variant item %r: no module step_amd.%s" % (item, mod))
                if not hasattr(m, attr):
                    raise ValueError("variant item %r: step_amd.%s has no attribute %s" % (item, mod, attr))
                old = getattr(m, attr)
                try:
                    new = ast.literal_eval(val)
                except (ValueError, SyntaxError):
                    raise ValueError("variant item %r: %r is not a Python literal" % (item, val))
                if type(old) is bool and type(new) is int and new in (0, 1):
                    new = bool(new)                      # (flag_ab.py's recorded spelling of a bool switch)
                elif type(old) is float and type(new) is int:
                    new = float(new)
                if old is not None and type(new) is not type(old):       # (an attribute that holds None takes any literal)
                    raise ValueError("variant item %r: step_amd.%s.%s is a %s, not a %s" % (item, mod, attr, type(old).__name__, type(new).__name__))
                switches.append((mod, attr, new))
            else:
                name = key[4:] if key.startswith("opt:") else key
                if name not in _capi.OPTION_IDS:
                    raise ValueError("variant item %r: no planner option %r (known: %s)" % (item, name, ", ".join(_capi.OPTION_IDS)))
                try:
                    options[name] = int(val)
                except ValueError:
                    raise ValueError("variant item %r: a planner option takes an integer" % item)
        return cls(text or "default", lib, options, tuple(switches))

    @classmethod
    def arg(cls, text):
        """Variant.parse as an argparse `type=`: the parse error becomes the usage error"""
        try:
            return cls.parse(text)
        except ValueError as e:
            raise argparse.ArgumentTypeError(str(e))

    @contextlib.contextmanager
    def applied(self):
        """inside: the variant's library is _lib.lib(), with its default options + the variant's, and the module switches are set;
        on exit (an exception included) the library handle, that library's options and every attribute are what they were"""
        L = load_build(self.lib) if self.lib else _lib.lib()
        mods = [importlib.import_module("step_amd." + mod) for mod, _, _ in self.switches]
        saved_options = _options_of(L)
        saved_attrs = [(m, attr, getattr(m, attr)) for m, (_, attr, _) in zip(mods, self.switches)]
        try:
            with _lib.use(L):
                L.step_reset_options()
                for k, v in self.options.items():
                    _capi.set_option(L, k, v)
                for m, (_, attr, v) in zip(mods, self.switches):
                    setattr(m, attr, v)
                yield L
        finally:
            for m, attr, old in reversed(saved_attrs):
                setattr(m, attr, old)
            for k, v in saved_options.items():
                _capi.set_option(L, k, v)


# ---- the captured step ------------------------------------------------------------------------------------------------------------------
def streams(n, device=None):
    """bench.py's arrangement for n batches: the default stream, then n - 1 side streams"""
    return [torch.cuda.current_stream(device)] + [torch.cuda.Stream(device) for _ in range(n - 1)]


def capture_step(fn, inputs, streams):
    """`fn(x)` (any callable from an input to an output tensor) as one HIP graph per input: two eager calls on the batch's stream, then
    the capture -- batch 0 on torch's own capture stream (it is replayed on the default stream), batch b on streams[b].
    -> (graphs, outputs), the outputs being the graphs' static output tensors"""
    graphs, outputs = [], []
    with torch.no_grad():
        for b, x in enumerate(inputs):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(streams[b]):
                for _ in range(2):
                    fn(x)
                torch.cuda.synchronize()
            if b == 0:
                with torch.cuda.graph(g):
                    y = fn(x)
            else:
                with torch.cuda.stream(streams[b]), torch.cuda.graph(g, stream=streams[b]):
                    y = fn(x)
            graphs.append(g)
            outputs.append(y)
    return graphs, outputs


def replay_ms(graphs, streams, in_flight, steps, warm=20):
    """ms per step: `warm` replays of batch 0, then `steps` replays round-robin over the first `in_flight` batches, each on its stream"""
    for _ in range(warm):
        graphs[0].replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        i = k % in_flight
        with torch.cuda.stream(streams[i]):
            graphs[i].replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


class Times(list):
    """the per-round times of one variant and leg, sorted"""
    median = property(lambda self: self[len(self) // 2])
    min = property(lambda self: self[0])


def interleave(variants, legs, rounds):
    """legs = {name: fn(variant) -> ms}; every round visits every variant in turn and runs each leg on it.
    -> one {leg name: Times} per variant, in the variants' order (by position: equal variants stay apart)"""
    res = [{name: [] for name in legs} for _ in variants]
    for _ in range(rounds):
        for r, v in zip(res, variants):
            for name, leg in legs.items():
                r[name].append(leg(v))
    return [{name: Times(sorted(t)) for name, t in r.items()} for r in res]


def same_bits(a, b):
    """(bit-identical?, max abs difference)"""
    return bool(torch.equal(a, b)), float((a.float() - b.float()).abs().max())


def ab_step(fn, inputs, variants, in_flight=(1, 2), rounds=5, steps=300):
    """the whole A/B: `fn` captured under every variant, batch 0's output compared with the first variant's, then the replays of
    `in_flight` batches interleaved.  -> ([same_bits vs the first variant], [{n in flight: Times}]), both in the variants' order"""
    ss = streams(max(max(in_flight), 1))
    inputs = inputs[:len(ss)]
    caps = []
    for v in variants:
        with v.applied():
            caps.append(capture_step(fn, inputs, ss))
    torch.cuda.synchronize()
    outs = []
    for graphs, ys in caps:
        graphs[0].replay()
        torch.cuda.synchronize()
        outs.append(ys[0].clone())
    legs = {n: (lambda cap, n=n: replay_ms(cap[0], ss, n, steps)) for n in in_flight}
    return [same_bits(o, outs[0]) for o in outs], interleave(caps, legs, rounds)


# ---- timers -----------------------------------------------------------------------------------------------------------------------------
def event_ms(fn, iters, warm=0):
    """ms per call: device events around `iters` back-to-back calls, after `warm` calls and a synchronise"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def wall_ms(fn, n, warm=0):
    """ms per call: the host clock around `n` calls between two synchronises, after `warm` calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


class tee:
    """say = tee(path): say(text) prints and keeps the line; say.close() writes the lines to `path` (None: nowhere)"""

    def __init__(self, path=None):
        self.path, self.lines = path, []

    def __call__(self, text=""):
        print(text, flush=True)
        self.lines.append(text)

    def close(self):
        if self.path:
            os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
            with open(self.path, "w") as f:
                f.write("\n".join(self.lines) + "\n")
