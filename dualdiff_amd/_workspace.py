"""Grow-only scratch buffers of the launches (split-K slabs, GroupNorm partials) and their graph-capture rules."""
import os
import threading

import torch

_WS = {}
_WS_MIN_BYTES = 64 << 20
_WS_IN_GRAPH = set()      # keys whose current buffer a captured HIP graph holds a raw pointer to
_WS_RETIRED = []          # such buffers after they were outgrown: kept alive for the graphs that use them
_WS_OWNER = threading.local()

# diagnostic builds (-DDD_DBG_STAMP, tools/build_dbg_libs.sh) write phase stamps into the tail of the workspace
_DBG_STAMP_WS = os.environ.get("DD_DBG_STAMP_WS", "0") == "1"


class workspace_owner:
    """`with workspace_owner(token):` scratch buffers handed out inside are keyed by `token` instead of the current
    stream's handle.  model_base.ForwardGraphs records each model's graphs under its own token: torch's stream handles
    are pooled and re-used, so two models' capture streams can share a handle — harmless while forward graphs replay one
    after the other, a race once two models' graphs replay concurrently (round 6: sibling overlap)."""

    def __init__(self, token):
        self.token = token

    def __enter__(self):
        self.prev = getattr(_WS_OWNER, "token", None)
        _WS_OWNER.token = self.token

    def __exit__(self, *exc):
        _WS_OWNER.token = self.prev


def workspace(nbytes, device, kind="gemm"):
    """Grow-only fp32 scratch buffer per (device, stream — or workspace_owner token —, kind): kernels on concurrent
    streams must not share scratch, and the split-K buffer (whose leading counter region dd_gemm keeps at zero)
    is never lent to GroupNorm.  Zero-filled on allocation; allocate before graph capture.
    A buffer that was handed out during a capture is never freed (torch's stream handles are pooled and
    re-used, so a later, larger eager workload can outgrow a buffer that a live graph still writes to)."""
    owner = getattr(_WS_OWNER, "token", None)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream().cuda_stream if owner is None else ("owner", owner), kind)
    ws = _WS.get(key)
    need = max(int(nbytes), _WS_MIN_BYTES)
    capturing = torch.cuda.is_current_stream_capturing()
    if ws is None or ws.numel() * 4 < need:
        if capturing:
            raise RuntimeError("workspace would have to grow during graph capture; run one eager "
                               "warm-up step first")
        if ws is not None and key in _WS_IN_GRAPH:
            _WS_RETIRED.append(ws)
            _WS_IN_GRAPH.discard(key)
        ws = torch.zeros((need + 3) // 4, dtype=torch.float32, device=device)
        _WS[key] = ws
    if capturing:
        _WS_IN_GRAPH.add(key)
    return ws


def attach(d, device, nbytes):
    """Gives the GEMM / conv descriptor `d` the split-K scratch its launch needs: `nbytes()` is asked after the tile and
    split-K of `d` are set.  Returns the byte count (0: the launch takes no scratch)."""
    need = nbytes()
    if need > 0 or _DBG_STAMP_WS:
        ws = workspace(need, device)
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    return need
