"""Parameter-gradient launches of a backward beside its data-gradient path (both backbones, roi_heads.py, rpn.py)."""
import os

import torch

_HEAD_WGRAD_STREAM = os.environ.get("SFOD_HEAD_WGRAD_STREAM", "1") != "0"      # 0: everything on one stream (A/B hook)


_shared = {}


def shared_stream():
    """ONE side stream per device for everything that runs beside a data-gradient path (the backbones' weight gradients, the
    heads' parameter gradients, the RPN's backward): HIP multiplexes streams onto 4 hardware queues, and a stream per module
    (six streams in a step) cost the 1024 x 2048 configuration 4.5 % (profiles/round5/r5_prefetch_label_free_work.txt)."""
    dev = torch.cuda.current_device()
    st = _shared.get(dev)
    if st is None:
        st = _shared[dev] = torch.cuda.Stream()
    return st


def heads_on(t):
    """the ``on`` of the heads' and the RPN's OffChain: the SFOD_HEAD_WGRAD_STREAM switch, and gradients on a GPU"""
    return _HEAD_WGRAD_STREAM and t.is_cuda


class OffChain:
    """Launches of a backward beside its data-gradient path, the ONLY code that moves work to the side stream and back:
    ``run(fn, *reads)`` executes ``fn`` on the device's side stream once everything enqueued on the current stream so far is
    done (``after``: once that event is, instead); the tensors in ``reads`` live in the current stream's pool, so the
    allocator is told the side stream uses them and the caller may drop them before the join.  ``wait()`` makes the current
    stream wait for the side stream; ``join(*outs)`` does that and hands the results over.  ``on`` false (a caller's A/B
    switch, CPU tensors): plain calls."""

    def __init__(self, on):
        self.side = shared_stream() if on else None

    def _beside(self):
        """already ON the side stream (the RPN's whole backward runs there, and its own parameter gradients come through
        here): plain calls -- an event recorded on a stream and awaited by the same stream is a no-op eagerly (and a
        self-dependency inside a graph capture: what made hipStreamEndCapture crash in round 6's graph experiment)"""
        return self.side is not None and torch.cuda.current_stream() != self.side

    def run(self, fn, *reads, after=None):
        if not self._beside():
            return fn()
        if after is None:
            after = torch.cuda.Event()
            after.record()
        with torch.cuda.stream(self.side):
            self.side.wait_event(after)
            out = fn()
        for t_ in reads:
            if t_ is not None:
                t_.record_stream(self.side)
        return out

    def wait(self):
        if self._beside():
            torch.cuda.current_stream().wait_stream(self.side)

    def join(self, *outs):
        if self._beside():
            self.wait()
            main = torch.cuda.current_stream()
            for t_ in outs:
                if t_ is not None:
                    t_.record_stream(main)


# ---- a whole head's backward beside the other head's --------------------------------------------------------------------
# The RPN's and the ROI heads' backward passes are independent until their feature-map gradients are added; autograd runs
# them one after the other on one stream.  The trainer's weighted-loss node marks the point where every loss gradient
# exists (``mark_loss_grads_ready``); a head that finds the mark runs its whole backward on its side stream from THERE --
# not from wherever the main stream has got to -- and the main stream waits for it at the end.
_loss_grads_ready = None


def mark_loss_grads_ready(g):
    """``g``: the tensor the loss gradients are slices of.  The mark keeps ``g`` itself alive (so its storage cannot be
    handed to another tensor while the mark exists) and is valid for ONE backward: ``clear_loss_grads_mark`` (the trainers
    call it when ``backward()`` returns) or the first ``take`` drops it."""
    global _loss_grads_ready
    if heads_on(g):
        ev = torch.cuda.Event()
        ev.record()
        _loss_grads_ready = (ev, g, g.device)


def take_loss_grads_ready(grad):
    """the mark, if ``grad`` is a view of the very tensor it was made for (a mark of another backward or another device is
    dropped): the marked tensor is held by reference, so equal storage addresses mean the same live storage"""
    global _loss_grads_ready
    m, _loss_grads_ready = _loss_grads_ready, None
    if m is None or not grad.is_cuda or grad.device != m[2]:
        return None
    if grad.untyped_storage().data_ptr() != m[1].untyped_storage().data_ptr():
        return None
    return m[0]


def clear_loss_grads_mark():
    """after ``backward()``: a mark nobody consumed (a step without an RPN loss) must not survive into the next backward"""
    global _loss_grads_ready
    _loss_grads_ready = None
