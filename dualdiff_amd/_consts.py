"""Process-lifetime device constants built on the host: THE rule (DESIGN.md "Device constants").  Nothing else in the
package keys a cache by device or uploads a host-built constant."""
import threading

import torch

_CONSTS = {}                    # (key, device type, device index) -> tensor or tuple of tensors on that device
_LOCK = threading.Lock()


def device_const(key, device, build):
    """The constant `key` on `device` (a torch.device or a string; a CUDA device without an index is the current one,
    "cpu" has index None): what build() returns — a CPU tensor or a tuple of CPU tensors — copied there once.

    - Published when complete: the upload is a blocking copy and the entry enters the dict only after its bytes are on
      the device.  torch's pageable host-to-device copy synchronises the stream it ran on; that stream is synchronised
      once more here, once per key, so that the contract does not rest on how torch copies.  Every stream of every thread
      that can see an entry may therefore read it: no event, no per-stream key, no device-side fill.
    - Capture: a miss on a CUDA device while the current stream is capturing raises RuntimeError before any HIP call (an
      upload would invalidate the capture); model_base.ForwardGraphs.call turns that into "this key runs eagerly".  A hit
      inside a capture is served.  For a CPU device the capture state is not asked.
    - Entries are never evicted or replaced: recorded graphs hold their addresses (ops.xattn_pack_weight).
    - A hit is a dict lookup without a lock; a miss builds under one, so one key is built once."""
    if not isinstance(device, torch.device):
        device = torch.device(device)
    cuda, index = device.type == "cuda", device.index
    if cuda and index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    k = (key, device.type, device.index)
    hit = _CONSTS.get(k)
    if hit is None:
        with _LOCK:
            hit = _CONSTS.get(k)
            if hit is None:
                if cuda and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("device constant %r on %s first requested inside a stream capture: "
                                       "run the call once eagerly before capturing it" % (key, device))
                host = build()
                parts = host if isinstance(host, tuple) else (host,)
                if not parts or not all(isinstance(t, torch.Tensor) and t.device.type == "cpu" for t in parts):
                    raise TypeError("device constant %r: build() must return a CPU tensor or a tuple of them" % (key,))
                parts = tuple(t.contiguous().to(device) for t in parts)
                if cuda:
                    torch.cuda.current_stream(device).synchronize()
                hit = _CONSTS[k] = parts if isinstance(host, tuple) else parts[0]
    return hit
