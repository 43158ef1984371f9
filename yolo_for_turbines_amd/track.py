"""Multi-object tracking on the device (``yolo_track_update``, csrc/track.hip): per stream a table of Kalman-filtered tracks that
one call per frame associates with the frame's detections by IoU, ByteTrack's way. The arithmetic and the order of a call are
defined to the bit in include/yolo_mi355x.h and DESIGN.md 7.23; nothing here computes."""
from __future__ import annotations

import collections
import math

import torch

from . import _lib as L
from .boxes import _nms_options, detect

__all__ = ["Tracker", "TrackResult", "track_images"]

TrackResult = collections.namedtuple("TrackResult", "boxes ids count det_ids")
TrackResult.__doc__ = """What :meth:`Tracker.update` returns: ``boxes`` (B, max_tracks, 6) rows [x, y, w, h, score, cls] and ``ids``
(B, max_tracks) int32 of the confirmed tracks seen in this frame, ascending id, the first ``count[b]`` of stream b (zero behind);
``det_ids`` (B, N) int32, per input row the id of the track it updated or founded (negative: the track is still tentative; 0: none)."""

MAX_STREAMS, MAX_TRACKS = 2047, 512                       # the limits of yolo_track_update
_HDR, _SLOT = 4, 26                                      # 32-bit words per stream and per slot of the state buffer


def _threshold(name, v):
    v = float(v)
    if not v >= 0.0 or math.isinf(v):
        raise ValueError(f"{name} must be a finite number >= 0, got {v}")
    return v


class Tracker:
    """ByteTrack-style tracker for ``streams`` independent streams (cameras or clips), all advanced by one :meth:`update` per frame.

    A detection above ``high_threshold`` is matched to the confirmed and lost tracks (IoU > ``match_iou[0]``); one between
    ``low_threshold`` and ``high_threshold`` can only continue a confirmed track (``match_iou[1]``); a track founded by a detection
    above ``new_threshold`` is tentative until it is matched again in the next frame (``match_iou[2]``), except in the first frame.
    A track unseen for more than ``max_age`` frames is dropped. Tracks keep the class of their founder and, unless
    ``class_agnostic``, only take detections of that class. All state is one device buffer; no call synchronises with the host, so
    :meth:`update` can be captured in ``torch.cuda.graph``."""

    def __init__(self, streams, max_tracks=128, high_threshold=0.5, low_threshold=0.1, new_threshold=0.6, match_iou=(0.2, 0.5, 0.3),
                 max_age=30, class_agnostic=False, box_format="center", device=None):
        for name, v, top in (("streams", streams, MAX_STREAMS), ("max_tracks", max_tracks, MAX_TRACKS)):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= top:
                raise ValueError(f"{name} must be an integer in [1, {top}], got {v!r}")
        self.streams, self.max_tracks = streams, max_tracks
        self.device = None if device is None else torch.device(device)
        self._state = self._ws = None
        self._set_params(high_threshold, low_threshold, new_threshold, match_iou, max_age, class_agnostic, box_format)

    def _set_params(self, high_threshold, low_threshold, new_threshold, match_iou, max_age, class_agnostic, box_format):
        high, low, new = (_threshold(n, v) for n, v in (("high_threshold", high_threshold), ("low_threshold", low_threshold),
                                                         ("new_threshold", new_threshold)))
        if not low <= high <= new:
            raise ValueError(f"thresholds must satisfy low <= high <= new, got {low}, {high}, {new}")
        try:
            match_iou = tuple(float(m) for m in match_iou)
        except TypeError:
            raise ValueError(f"match_iou must be three numbers, got {match_iou!r}") from None
        if len(match_iou) != 3 or not all(0.0 <= m <= 1.0 for m in match_iou):
            raise ValueError(f"match_iou must be three numbers in [0, 1], got {match_iou!r}")
        if isinstance(max_age, bool) or int(max_age) != max_age or max_age < 0:
            raise ValueError(f"max_age must be an integer >= 0, got {max_age!r}")
        if box_format not in ("center", "corners"):
            raise ValueError(f"box_format must be 'center' or 'corners', got {box_format!r}")
        self.high_threshold, self.low_threshold, self.new_threshold, self.match_iou = high, low, new, match_iou
        self.max_age, self.class_agnostic, self.box_format = int(max_age), bool(class_agnostic), box_format
        self._params = L.TrackParams(high, low, new, (L.C.c_double * 3)(*match_iou), self.max_age, int(box_format == "center"),
                                     int(self.class_agnostic), 0)

    def _params_dict(self):
        return dict(high_threshold=self.high_threshold, low_threshold=self.low_threshold, new_threshold=self.new_threshold,
                    match_iou=self.match_iou, max_age=self.max_age, class_agnostic=self.class_agnostic, box_format=self.box_format)

    # ---- the state buffer
    def _buffer(self, device=None):
        """The state tensor (streams, 4 + 26 max_tracks) int32, allocated and reset on first use."""
        if self._state is None:
            dev = self.device or device or torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise RuntimeError("Tracker runs on MI355X only (no CPU fallback)")
            self.device = dev
            assert L.lib().yolo_track_state_bytes(self.streams, self.max_tracks) == 4 * self.streams * (_HDR + _SLOT * self.max_tracks)
            self._state = torch.empty((self.streams, _HDR + _SLOT * self.max_tracks), dtype=torch.int32, device=dev)
            self.reset()
        return self._state

    def reset(self, streams=None):
        """Forget the tracks of all streams, or of the stream indices in ``streams``; ids start at 1 again. Stream-ordered."""
        mask = None
        if streams is not None:
            host = torch.zeros(self.streams, dtype=torch.uint8)
            for s in streams:
                if isinstance(s, bool) or int(s) != s or not 0 <= s < self.streams:
                    raise ValueError(f"stream index {s!r} outside [0, {self.streams})")
                host[int(s)] = 1
        state = self._buffer()
        with torch.cuda.device(self.device):
            if streams is not None:
                mask = host.to(self.device)
            L.check(L.lib().yolo_track_reset(state.data_ptr(), self.streams, self.max_tracks, L.ptr(mask), L.current_stream()),
                    "yolo_track_reset")

    def slots(self):
        """The state decoded into tensors (views of the buffer): ``frame``, ``next_id``, ``overflow`` (B,); ``state`` (0 free,
        1 tentative, 2 tracked, 3 lost), ``id``, ``lost_frames`` (B, max_tracks) int32; ``cls``, ``score`` (B, max_tracks),
        ``mean`` (B, max_tracks, 8) = cx, cy, w, h and their velocities, ``cov`` (B, max_tracks, 12) fp32."""
        st = self._buffer()
        sl = st[:, _HDR:].view(self.streams, self.max_tracks, _SLOT)
        f = sl.view(torch.float32)
        return dict(frame=st[:, 0], next_id=st[:, 1], overflow=st[:, 2], state=sl[..., 0], id=sl[..., 1], cls=f[..., 2], score=f[..., 3],
                    lost_frames=sl[..., 4], mean=f[..., 5:13], cov=f[..., 13:25])

    def state_dict(self):
        return {"state": self._buffer().clone(), "streams": self.streams, "max_tracks": self.max_tracks, "params": self._params_dict()}

    def load_state_dict(self, sd):
        """Take over a :meth:`state_dict` (same ``streams`` and ``max_tracks``): the tracks and the parameters; the next
        :meth:`update` continues bit-identically."""
        if sd["streams"] != self.streams or sd["max_tracks"] != self.max_tracks:
            raise ValueError(f"state of {sd['streams']} streams x {sd['max_tracks']} tracks, tracker of {self.streams} x {self.max_tracks}")
        state = sd["state"]
        if state.dtype != torch.int32 or tuple(state.shape) != (self.streams, _HDR + _SLOT * self.max_tracks):
            raise ValueError("state buffer of the wrong type or shape")
        self._set_params(**sd["params"])
        self._buffer(state.device if state.is_cuda else None).copy_(state)

    # ---- one frame
    def update(self, boxes, keep=None, count=None):
        """One frame for every stream. ``boxes``: (streams, N, 6) fp32 CUDA rows [x, y, w, h, obj, cls] in the tracker's
        ``box_format``. With ``keep`` (streams, N) and ``count`` (streams,) int32, the output of :func:`detect` /
        :func:`nms_indices`, the detections are the rows ``boxes[s, keep[s, :count[s]]]``; with ``count`` alone (the output of
        :func:`fuse_boxes`) the first ``count[s]`` rows; with neither every row. Returns a :class:`TrackResult`. No host
        synchronisation."""
        if not isinstance(boxes, torch.Tensor) or boxes.dim() != 3 or boxes.shape[-1] != 6 or not boxes.is_floating_point():
            raise ValueError("boxes must be a floating-point (streams, N, 6) tensor")
        B, N, _ = boxes.shape
        if B != self.streams:
            raise ValueError(f"boxes of {B} streams, tracker of {self.streams}")
        if keep is not None and count is None:
            raise ValueError("keep needs count")
        for name, t, shape in (("keep", keep, (B, max(N, 1))), ("count", count, (B,))):
            if t is not None and (not isinstance(t, torch.Tensor) or t.is_floating_point() or tuple(t.shape) != shape):
                raise ValueError(f"{name} must be an integer tensor of shape {shape}")
        if not boxes.is_cuda or any(t is not None and not t.is_cuda for t in (keep, count)):
            raise RuntimeError("Tracker.update runs on MI355X only (no CPU fallback)")
        lib = L.lib()
        nbytes = lib.yolo_track_workspace_bytes(B, N, self.max_tracks)
        if N and nbytes == 0:
            raise ValueError(f"update takes at most 163,456 boxes per stream, got {N}")
        state = self._buffer(boxes.device)
        if boxes.device != self.device:
            raise ValueError(f"boxes on {boxes.device}, tracker on {self.device}")
        boxes = boxes.float().contiguous()
        keep = None if keep is None or N == 0 else keep.to(torch.int32).contiguous()
        count = None if count is None else count.to(torch.int32).contiguous()
        dev, M = self.device, self.max_tracks
        with torch.cuda.device(dev):
            out_boxes = torch.empty((B, M, 6), dtype=torch.float32, device=dev)
            out_ids = torch.empty((B, M), dtype=torch.int32, device=dev)
            out_count = torch.empty((B,), dtype=torch.int32, device=dev)
            det_ids = torch.empty((B, N), dtype=torch.int32, device=dev)
            if self._ws is None or self._ws.numel() < nbytes:        # the tracker's own: a captured update keeps its address
                self._ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
            L.check(lib.yolo_track_update(state.data_ptr(), B, M, boxes.data_ptr(), N, L.ptr(keep), L.ptr(count), L.C.byref(self._params),
                                          out_boxes.data_ptr(), out_ids.data_ptr(), out_count.data_ptr(), det_ids.data_ptr(),
                                          self._ws.data_ptr(), self._ws.numel(), L.current_stream()), "yolo_track_update")
        return TrackResult(out_boxes, out_ids, out_count, det_ids)


def track_images(model, x, scaled_anchors, tracker, iou_threshold=0.45, nms=None):
    """One frame per stream from pixels to tracks: :func:`detect_images` with ``obj_threshold = tracker.low_threshold`` (so the low
    detections survive the NMS for the tracker's second matching), then :meth:`Tracker.update` on its (boxes, keep, count). One
    host synchronisation, the forward's NaN guard, after everything is enqueued. Returns ``(TrackResult, boxes, keep, count)``.
    ``nms``: as for :func:`detect`; its ``score_threshold`` defaults to ``tracker.low_threshold`` too. With Soft-NMS an overlapped
    detection reaches the tracker with its lowered objectness instead of being removed: a box behind a confident one falls from
    HIGH to LOW and is offered to the second matching."""
    if not isinstance(tracker, Tracker):
        raise ValueError("tracker must be a Tracker")
    if tracker.box_format != "center":
        raise ValueError("track_images decodes centre-format boxes: the tracker must have box_format='center'")
    if nms is not None:
        _nms_options(nms, tracker.low_threshold)          # a bad option is reported before the forward runs
    eng = model._engine
    with eng.deferred_nan(), torch.no_grad():
        preds = model(x)
        flag = eng.take_pending_flag()
    boxes, keep, count = detect(preds, scaled_anchors, iou_threshold, tracker.low_threshold, "center", nms=nms)
    res = tracker.update(boxes, keep, count)
    if flag is not None:
        eng.raise_on_nan(flag)
    return res, boxes, keep, count
