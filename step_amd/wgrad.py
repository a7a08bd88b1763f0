"""step_amd/wgrad.py -- the route a conv unit's weight gradient takes during backward, and the one object that owns the state of that path.  Routes:
`into` (inside wgrad_into_grad(): accumulated into the parameter's .grad on a side stream nobody waits for until sync()), `beside` (fp32 per-unit nodes:
on the side stream beside the data-gradient conv, joined right behind it) or inline.  Who arms, who disarms, when the queue flushes: DESIGN.md 3, at its end."""
from typing import Any, NamedTuple

import torch

from . import ops

WGRAD16 = True            # 16-bit activations: weight gradients on the 16-bit MFMA (step_conv_wgrad16)
WGRAD_SIDE_STREAM = True  # training: weight gradient beside the data gradient
BESIDE = "beside"         # WgradState.route(): on the side stream, returned


class Pending(NamedTuple):   # one deferred fixed-order sum of partial tiles (ops.conv_wgrad_partial)
    item: Any             # the _capi.WgradReduceItem of the sum
    ws: Any               # its workspace: alive until the sum has been launched
    unit: Any             # the ConvUnit to announce to the gradient exchange then (None: the gradient goes back through autograd)
    stream: Any           # the side stream the partial tiles were written on (None: the current stream)
    device: Any


class WgradState:
    """The live state of the weight gradients of a backward pass.  PROCESS-GLOBAL: exactly one instance (STATE) serves every model,
    device and thread of the process -- one backward pass at a time uses it, as one gradient exchange at a time is armed."""
    def __init__(self):
        self.into_grad = False     # see wgrad_into_grad()
        self.ready = self.defer = None   # the armed exchange's BucketedReducer.ready / .defer (defer: flush() will announce the parameter, not autograd's hook)
        self.in_flight = False     # the side stream holds accumulations the main stream has not waited for
        self.queue = []            # deferred sums of the per-unit nodes (flushed eight at a time and in sync())
        self.keep = []             # tensors the side stream reads that autograd must not modify in place (until sync())
        self.streams = {}          # (device type, index) -> the two side streams

    def side_streams(self, device):
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        return self.streams.get(key) or self.streams.setdefault(key, (torch.cuda.Stream(device), torch.cuda.Stream(device)))

    def arm(self, ready, defer):                                 # a gradient exchange wants to hear about the gradients of the coming backward pass
        self.ready, self.defer = ready, defer

    def disarm(self, ready=None):                                # with `ready`: only when that exchange is the armed one
        if ready is None or self.ready is ready:
            self.ready = self.defer = None

    @staticmethod
    def use16(x, gdtype):                                        # 16-bit activations and their gradient in the same dtype: the 16-bit MFMA
        return WGRAD16 and x.dtype != torch.float32 and gdtype == x.dtype

    @staticmethod
    def target(unit, w_eff):
        """The dense fp32 .grad of the unit's weight parameter when the effective weight IS that parameter (no channel slice /
        permutation) and a gradient buffer exists; else None (the caller returns the gradient through autograd)."""
        if unit.cin_slice is not None or unit.perm is not None:
            return None
        w = unit.weight_fn()
        g = w.grad
        ok = g is not None and g.dtype == torch.float32 and g.is_contiguous() and g.numel() == w_eff.numel() and w.requires_grad
        return g if ok else None

    def route(self, unit, w_eff, x, beside=False):               # the .grad to accumulate into | BESIDE (a caller that launches a data gradient next and join()s) | None
        target = self.target(unit, w_eff) if (self.into_grad and x.is_cuda and ops.PROFILE is None) else None
        side = beside and WGRAD_SIDE_STREAM and x.is_cuda and x.dtype == torch.float32 and ops.PROFILE is None
        return BESIDE if (target is None and side) else target

    def unit_wgrad(self, unit, w_eff, x, g, k, pend=None, route=None):
        """Weight gradient of one conv unit from its input x and the gradient g of its conv output (both channels-last, g possibly a channel
        slice), on route(unit, w_eff, x) unless the caller passes the route it asked for: `into` returns None, the others the gradient.  pend (a list):
        the sum of the partial tiles is deferred and described there -- flush() runs a block's sums as one launch (and only then announces them)."""
        w16 = self.use16(x, g.dtype)
        if not w16 and g.dtype != torch.float32:
            g = g.float()
        fn = ops.conv_wgrad16 if w16 else ops.conv_wgrad
        cout = w_eff.shape[0]
        target = self.route(unit, w_eff, x) if route is None else route
        defer = pend is not None and ops.PROFILE is None and (ops.WGRAD16_WS if w16 else ops.WGRAD_WS)
        if target is None:
            if defer:
                dw, item, ws = ops.conv_wgrad_partial(x, g, cout, k)
                pend.append(Pending(item, ws, None, None, x.device))
                assert dw.dtype == w_eff.dtype                   # (fp32 master weights: a cast here would read the gradient before its sum has run)
                return dw
            return fn(x, g, cout, k).to(w_eff.dtype)
        side = self.side_streams(x.device)[0]
        side.wait_stream(torch.cuda.current_stream(x.device))
        with torch.cuda.stream(side):
            if target is BESIDE:
                # (C4 fp32 69.3 -> 65.0 ms; 16-bit data-gradient convs are too short to hide anything, 46.1 -> 47.2 ms, and stay on one stream)
                return fn(x, g, cout, k).to(w_eff.dtype)
            if defer:
                _, item, ws = ops.conv_wgrad_partial(x, g, cout, k, into=target)
                pend.append(Pending(item, ws, unit, side, x.device))
                if self.defer is not None:
                    self.defer(unit.weight_fn())
            else:
                fn(x, g, cout, k, into=target)
        x.record_stream(side)
        g.record_stream(side)
        self.in_flight = True
        if self.ready is not None and not defer:                 # this parameter bypasses autograd's accumulate hook
            self.ready(unit.weight_fn(), side)

    def join(self, gw):                                          # behind the data gradient of a BESIDE route: the current stream waits for gw
        main = torch.cuda.current_stream(gw.device)
        main.wait_stream(self.side_streams(gw.device)[0])
        gw.record_stream(main)

    def flush(self, pend=None):
        """The deferred sums of unit_wgrad(pend=...) (default: the queue), one launch (per eight layers); then the exchange hears about the parameters."""
        pend = self.queue if pend is None else pend
        # One launch PER STREAM the partial tiles were written on (None = the current stream, whose dw autograd reads next: its sum
        # must be ordered on that stream, not on the side stream of a neighbour that happens to have a dense fp32 .grad).
        parts = {}
        for e in pend:
            parts.setdefault((e.device, e.stream), []).append(e)
        for (dev, side), es in parts.items():
            items = [e.item for e in es]
            if side is None:
                ops.wgrad_reduce_group(items, dev)
                continue
            with torch.cuda.stream(side):
                ops.wgrad_reduce_group(items, dev)
            for e in es:
                if e.ws is not None:
                    e.ws.record_stream(side)
                if self.ready is not None and e.unit is not None:
                    self.ready(e.unit.weight_fn(), side)
        del pend[:]

    def sync(self):
        """Order every weight gradient launched on the side stream before what the current stream does next."""
        self.flush()
        if self.in_flight and torch.cuda.is_available():
            for dev_key, streams in list(self.streams.items()):
                torch.cuda.current_stream(torch.device(dev_key[0], dev_key[1])).wait_stream(streams[0])
            self.in_flight = False
        del self.keep[:]


STATE = WgradState()
wgrad_sync = STATE.sync


class wgrad_into_grad:
    """Context manager for a training step whose optimizer owns persistent gradient buffers (step_amd.optim.FlatAdam): inside it the conv units
    add their weight gradients into `weight.grad` directly, asynchronously on a side stream.  Leaving the context (or calling wgrad_sync())
    makes the current stream wait for them.  Not for torch.autograd.grad() or double backward: the weight gradient bypasses autograd."""
    def __enter__(self):
        if not STATE.into_grad:
            STATE.sync()                                         # nothing of an earlier backward may ride into this step's sums
        self.prev, STATE.into_grad = STATE.into_grad, True
        return self

    def __exit__(self, *exc):
        STATE.into_grad = self.prev
        if exc and exc[0] is not None:
            # backward raised mid-way: the queued sums describe a gradient nobody will use -- dropped, not added to the arena at the next flush;
            # the side stream is still joined.  This step's gradients are UNDEFINED (zero the arena before the next backward), and the exchange is
            # disarmed so that a BucketedReducer armed for this step does not wait for parameters that will never report (its begin() re-arms).
            del STATE.queue[:]
            STATE.disarm()
        STATE.sync()
