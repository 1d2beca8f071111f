"""Captured steps: the stateless ops of ``ss_amd.ops`` recorded into a ``torch.cuda.CUDAGraph`` and replayed
(include/ss_hip.h "Captured steps").

The library keeps its scratches - the stash of ``k_obs_rows``, the hand-off area of ``k_obs_blocks`` - per (device, stream), and
what a stream's first call allocates cannot be allocated inside a capture.  So ``capture`` prepares ONE side stream (by
``ss_stream_reserve``, or by running the step once eagerly there), captures the step on that same stream as one linear chain, and
replays it there.  The context entries (``ss_amd.context``) are not served: their descriptor ring waits on events on the host.

    step = lambda: (ops.source_windows_into(clip, win_desc, spec),
                    ops.audio_obs_into(spec, bank, lens, unit_desc, None, sgram, 44100, 44100))
    cap = graphs.capture(step, reserve=dict(out_len=44100, rir_cap=bank.shape[2], n_terms=2))
    for _ in range(steps):
        unit_desc.copy_(next_desc, non_blocking=True)      # inputs are rewritten IN PLACE: the graph holds their addresses
        cap.replay()                                       # sgram is ready for the current stream
"""
from __future__ import annotations

import ctypes
from typing import Callable, Optional

import torch

from . import _lib


class Captured:
    """A captured step.  ``stream``: the side stream it was captured on and replays on; eager calls that share its scratches
    belong on that stream too (``with torch.cuda.stream(cap.stream)``)."""

    def __init__(self, graph: "torch.cuda.CUDAGraph", stream: "torch.cuda.Stream"):
        self.graph = graph
        self.stream = stream

    def replay(self, fence: bool = True) -> None:
        """One replay on ``stream``.  fence: the replay waits for the work the current stream has queued (the in-place writes of
        its inputs) and the current stream waits for the replay; ``fence=False`` leaves both to the caller."""
        cur = torch.cuda.current_stream(self.stream.device)
        if fence and cur != self.stream:
            self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            self.graph.replay()
        if fence and cur != self.stream:
            cur.wait_stream(self.stream)

    def replay_epoch(self) -> int:
        """``ss_stream_replay_epoch``: synchronises ``stream``; 0 = no replay of a k_obs_blocks launch yet, -k after the k-th.
        Raises when the stream has no hand-off area (no such launch was ever prepared on it)."""
        out = ctypes.c_int(0)
        with torch.cuda.device(self.stream.device):
            _lib.check(_lib.load().ss_stream_replay_epoch(self.stream.cuda_stream, ctypes.byref(out)), "ss_stream_replay_epoch")
        return out.value


def capture(fn: Callable[[], object], *, stream: Optional["torch.cuda.Stream"] = None, reserve: Optional[dict] = None) -> Captured:
    """Capture ``fn()`` - calls of the stateless ops on the current stream, nothing that synchronises or allocates - into a graph.

    stream: the side stream to capture and replay on (never the default stream); made here when None.
    reserve: ``dict(out_len=, rir_cap=, n_terms=)`` for ``ss_stream_reserve`` - the stream is prepared without running the step.
    Without it ``fn()`` runs once eagerly on the stream first (its outputs are written once before the first replay).
    The tensors ``fn`` reads and writes must stay alive and in place for as long as the graph is replayed."""
    if stream is None:
        stream = torch.cuda.Stream()
    cur = torch.cuda.current_stream(stream.device)
    if cur == stream or stream == torch.cuda.default_stream(stream.device):
        raise ValueError("capture needs a side stream: not the current stream, not the device's default stream")
    stream.wait_stream(cur)                                 # whatever has prepared the step's inputs
    with torch.cuda.device(stream.device):
        if reserve is not None:
            _lib.check(_lib.load().ss_stream_reserve(stream.cuda_stream, int(reserve["out_len"]), int(reserve["rir_cap"]),
                                                     int(reserve["n_terms"])), "ss_stream_reserve")
        else:
            with torch.cuda.stream(stream):
                fn()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            fn()
    return Captured(graph, stream)
