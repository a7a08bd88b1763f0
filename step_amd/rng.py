"""step_amd/rng.py -- the device-side random generator behind step_amd.Dropout (include/step_amd.h: step_dropout_forward).

The state is two 64-bit words ON THE DEVICE, {seed, offset}: the kernels read it there and a one-thread kernel behind each dropout
pass increments the offset, so successive calls -- and successive replays of a captured graph -- draw new masks without the host.
The host writes the state only when it seeds or restores it, never inside a capture."""
import torch

_M64 = (1 << 64) - 1


def _signed(v):
    v &= _M64
    return v - (1 << 64) if v >= (1 << 63) else v


class DeviceRNG:
    """One generator: `state` is an int64[2] tensor on `device` holding {seed, offset} (as unsigned 64-bit patterns)."""

    def __init__(self, device, seed=0):
        self.device = torch.device(device)
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.set_state((seed, 0))

    def manual_seed(self, seed):
        """seed the stream and rewind it: {seed, offset 0}"""
        self.set_state((seed, 0))
        return self

    def set_state(self, state):
        """(seed, offset) host integers -> the device (a checkpoint's get_state()); refused while the current stream is capturing"""
        seed, offset = (int(v) for v in state)
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("step_amd.rng: the generator state cannot be written from the host inside a graph capture "
                               "(seed before capture(); the captured step advances the offset on the device)")
        self.state.copy_(torch.tensor([_signed(seed), _signed(offset)], dtype=torch.int64))

    def get_state(self):
        """(seed, offset) as host integers; synchronises"""
        s = self.state.cpu().tolist()
        return (s[0] & _M64, s[1] & _M64)

    def offset(self):
        """how many dropout passes the stream has served since it was seeded; synchronises (tests, the launcher's summary)"""
        return self.get_state()[1]


_DEFAULT = {}
_SEED = 0


def _key(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def default(device):
    """the per-device generator step_amd.Dropout draws from (created on first use with the seed of the last manual_seed)"""
    device = _key(device)
    g = _DEFAULT.get(device)
    if g is None:
        g = _DEFAULT[device] = DeviceRNG(device, _SEED)
    return g


def manual_seed(seed):
    """Seed every existing and every future default generator with `seed`, offset 0 (what torch.manual_seed is to torch's generators)."""
    global _SEED
    _SEED = int(seed)
    for g in _DEFAULT.values():
        g.manual_seed(_SEED)
