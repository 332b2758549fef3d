"""`Engine`: one fpc_ctx (one GPU, one frame geometry) behind a small Python class.

PyTorch is used for what it is good at here -- owning device memory and streams;
all arithmetic happens inside libfpc.so.  Tensors cross the boundary as raw
device pointers (`tensor.data_ptr()`).
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, arch


def _as_tensor_table(state_dict):
    """{name: array-like} -> (FpcTensor[n], keep-alive list).  Only float entries go in
    (`num_batches_tracked` is an int64 counter the path never reads)."""
    keep, items = [], []
    for name, v in state_dict.items():
        if isinstance(v, torch.Tensor):
            if not v.dtype.is_floating_point:
                continue
            v = v.detach().cpu().contiguous().float().numpy()
        else:
            v = np.asarray(v)
            if v.dtype.kind != "f":
                continue
            v = np.ascontiguousarray(v, dtype=np.float32)
        if v.ndim > 4:
            raise ValueError("tensor %s has %d dims" % (name, v.ndim))
        keep.append(v)
        items.append((name.encode(), v))
    table = (_lib.FpcTensor * len(items))()
    for i, (name, v) in enumerate(items):
        table[i].name = name
        table[i].data = v.ctypes.data
        table[i].ndim = v.ndim
        for d in range(v.ndim):
            table[i].shape[d] = v.shape[d]
    keep.append(items)
    return table, keep


class Engine:
    def __init__(self, height, width, max_batch=1, device=0, nms_dist=4, conf_thresh=0.015,
                 border_remove=4, descriptor_enabled=True, max_keypoints=0, in_channels=3, dtype="f32", arch="resnet",
                 num_streams=0, plan_flags=(), nms_round_launches=0, min_sub_batch=0):
        self._l = _lib.load()          # raises if libfpc.so is not built: no fallback
        if not torch.cuda.is_available():
            raise RuntimeError("fpc_amd needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU path in the product")
        cfg = _lib.FpcConfig()
        _lib.check(self._l.fpc_default_config(ctypes.byref(cfg)), "fpc_default_config")
        cfg.device, cfg.height, cfg.width, cfg.max_batch = device, height, width, max_batch
        cfg.nms_dist, cfg.conf_thresh, cfg.border_remove = nms_dist, conf_thresh, border_remove
        cfg.descriptor_enabled, cfg.max_keypoints = int(bool(descriptor_enabled)), max_keypoints
        cfg.in_channels = in_channels
        codes = {"f32": 0, "bf16": 1, "f32_split": 2, "f32_split_f16": 3}   # FPC_F32 ... FPC_F32_SPLIT_F16 (include/fpc.h)
        if dtype not in codes:
            raise ValueError("dtype must be one of %s, got %r" % (sorted(codes), dtype))
        cfg.dtype = codes[dtype]
        self.dtype = dtype
        if arch not in ("resnet", "vgg"):
            raise ValueError("arch must be 'resnet' (python/src/superpoint.py) or 'vgg' (cpp/src/model.cc), got %r" % (arch,))
        cfg.arch = 1 if arch == "vgg" else 0     # FPC_ARCH_RESNET / FPC_ARCH_VGG
        self.arch = arch
        self.in_channels = 1 if in_channels == 1 else 3
        # launch-plan knobs (fpc_config.num_streams / plan_flags / ...; zeros = the default plan)
        cfg.num_streams, cfg.nms_round_launches, cfg.min_sub_batch = num_streams, nms_round_launches, min_sub_batch
        flags = 0
        for f in ([plan_flags] if isinstance(plan_flags, (str, int)) else plan_flags):
            flags |= f if isinstance(f, int) else _lib.PLAN_FLAGS[f]
        cfg.plan_flags = flags
        self.cfg = cfg
        self.h, self.w, self.max_batch, self.device = height, width, max_batch, device
        self.descriptor_enabled = bool(descriptor_enabled)
        self._ctx = ctypes.c_void_p()
        _lib.check(self._l.fpc_create(ctypes.byref(self._ctx), ctypes.byref(cfg)), "fpc_create")
        self.torch_device = torch.device("cuda", device)
        res = _lib.FpcDeviceResults()
        _lib.check(self._l.fpc_results(self._ctx, ctypes.byref(res)), "fpc_results")
        self.capacity, self.desc_dim = res.capacity, res.desc_dim
        self._res = res

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            bad = 0
            if os.environ.get("FPC_GUARD_ZONES") == "1":
                # a whole run under the canary zones (FPC_GUARD_ZONES=1 python -m pytest tests -m gpu): every context is
                # checked when it is closed, and a kernel that stored outside its tensors fails the test that closed it
                b = ctypes.c_longlong(0)
                if self._l.fpc_check_guards(self._ctx, ctypes.byref(b)) == 0:
                    bad = int(b.value)
            self._l.fpc_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()
            self._bank = None
            if bad:
                raise RuntimeError("fpc_check_guards: %d canary words were overwritten -- a kernel stored outside its tensors" % bad)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights ---------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        """Strict load of ckpt['model_state_dict'] (reference: saveutils.py:6-18)."""
        table, keep = _as_tensor_table(state_dict)
        _lib.check(self._l.fpc_load_weights(self._ctx, table, len(table)), "fpc_load_weights")
        del keep

    def packed_size(self):
        return self._l.fpc_packed_size(self._ctx)

    def packed_view(self):
        """The packed weight blob as a uint8 CUDA tensor aliasing the library's buffer
        (the in-place target of the RCCL broadcast, see dist.py)."""
        n = self.packed_size()
        ptr = self._l.fpc_packed_device_ptr(self._ctx)
        holder = _DevArray(ptr, n)
        return torch.as_tensor(holder, device=self.torch_device)

    def export_packed(self):
        buf = np.empty(self.packed_size(), np.uint8)
        _lib.check(self._l.fpc_export_packed(self._ctx, buf.ctypes.data, buf.nbytes), "fpc_export_packed")
        return buf

    def import_packed(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        _lib.check(self._l.fpc_import_packed(self._ctx, buf.ctypes.data, buf.nbytes), "fpc_import_packed")

    def import_packed_device(self, buf):
        """fpc_import_packed_device: a packed blob that is already in device memory (a uint8 CUDA tensor -- the receive
        buffer of a broadcast, another engine's packed_view()): tag checked, copied device to device."""
        if buf.dtype != torch.uint8 or not buf.is_cuda or not buf.is_contiguous():
            raise ValueError("import_packed_device takes a contiguous uint8 CUDA tensor")
        torch.cuda.synchronize(buf.device)
        _lib.check(self._l.fpc_import_packed_device(self._ctx, buf.data_ptr(), buf.numel()), "fpc_import_packed_device")

    def mark_weights_loaded(self):
        _lib.check(self._l.fpc_mark_weights_loaded(self._ctx), "fpc_mark_weights_loaded")

    def plan_hash(self):
        """Equal on two engines iff they can exchange packed weights (same build, dtype, arch, launch plan)."""
        return int(self._l.fpc_plan_hash(self._ctx))

    def broadcast_weights(self, nccl_comm, root=0):
        """fpc_broadcast_weights: RCCL broadcast of the packed blob on a raw ncclComm_t (an int / c_void_p)."""
        _lib.check(self._l.fpc_broadcast_weights(self._ctx, ctypes.c_void_p(nccl_comm), root), "fpc_broadcast_weights")

    # -- execution -------------------------------------------------------------------
    def use_torch_stream(self):
        s = torch.cuda.current_stream(self.torch_device).cuda_stream
        _lib.check(self._l.fpc_set_stream(self._ctx, ctypes.c_void_p(s)), "fpc_set_stream")

    def torch_stream(self):
        """The ctx's main stream as a torch stream (events recorded / awaited on it order torch work against fpc_detect)."""
        return torch.cuda.ExternalStream(int(self._l.fpc_get_stream(self._ctx)), device=self.torch_device)

    def upload_stream(self):
        """fpc_upload_stream: a stream for the caller's uploads that shares no hardware queue with the ctx's compute streams."""
        s = self._l.fpc_upload_stream(self._ctx)
        if not s:
            raise RuntimeError("fpc_upload_stream failed")
        return torch.cuda.ExternalStream(int(s), device=self.torch_device)

    def stream_report(self):
        """fpc_stream_report: which hardware queue each of the ctx's streams sits on, and what finding that out cost."""
        r = _lib.FpcStreamReport()
        _lib.check(self._l.fpc_stream_report(self._ctx, ctypes.byref(r)), "fpc_stream_report")
        names = {0: "main", 200: "upload"}
        streams = {}
        for i in range(r.n_streams):
            sl = r.slot[i]
            name = names.get(sl) or ("sub%d" % sl if sl < 100 else "side%d" % (sl - 100))
            streams[name] = r.queue[i]
        return {"streams": streams, "probing": bool(r.probing), "hw_queues_found": r.hw_queues_found,
                "create_probe_rounds": r.create_probe_rounds, "create_placement_ms": round(r.create_placement_ms, 3),
                "process_probe_rounds": r.process_probe_rounds, "process_probe_launches": r.process_probe_launches,
                "process_probe_ms": round(r.process_probe_ms, 3),
                "process_inconclusive_rounds": r.process_inconclusive_rounds,
                "process_registered_streams": r.process_registered_streams}

    def _frames(self, frames):
        if not isinstance(frames, torch.Tensor):
            frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32))
        frames = frames.to(self.torch_device, torch.float32).contiguous()
        if frames.dim() != 4 or frames.shape[1] != self.in_channels or frames.shape[2] != self.h or frames.shape[3] != self.w:
            raise ValueError("frames must be [n,%d,%d,%d], got %s" % (self.in_channels, self.h, self.w, tuple(frames.shape)))
        if frames.shape[0] > self.max_batch:
            raise ValueError("batch %d > max_batch %d" % (frames.shape[0], self.max_batch))
        return frames

    def forward(self, frames):
        """SuperPoint.forward (superpoint.py:91-115): -> prob_map [n,H,W], desc [n,128,H/8,W/8],
        logits [n,65,H/8,W/8] as CUDA tensors."""
        frames = self._frames(frames)
        n = frames.shape[0]
        dev = self.torch_device
        prob = torch.empty((n, self.h, self.w), device=dev)
        desc = torch.empty((n, self.desc_dim, self.h // 8, self.w // 8), device=dev)
        logits = torch.empty((n, 65, self.h // 8, self.w // 8), device=dev)
        torch.cuda.synchronize(dev)
        _lib.check(self._l.fpc_forward(self._ctx, frames.data_ptr(), n, prob.data_ptr(), desc.data_ptr(),
                                       logits.data_ptr()), "fpc_forward")
        self.sync()
        return prob, desc, logits

    def detect_async(self, frames_dev, n):
        """Enqueue the whole path for n device-resident frames (no sync, no copies)."""
        _lib.check(self._l.fpc_detect(self._ctx, frames_dev.data_ptr(), n), "fpc_detect")

    def detect(self, frames):
        frames = self._frames(frames)
        torch.cuda.synchronize(self.torch_device)
        self.detect_async(frames, frames.shape[0])
        return self.fetch(frames.shape[0])

    U8_LAYOUTS = {"gray": 0, "rgb_hwc": 1, "bgr_hwc": 2, "bgr_hwc_gray": 3}   # FPC_U8_* (include/fpc.h)

    def detect_u8_async(self, frames_u8_dev, n, layout):
        """8-bit device frames (camera.py:31: float32(u8) / 255.0, converted on the device) -> the whole path."""
        _lib.check(self._l.fpc_detect_u8(self._ctx, frames_u8_dev.data_ptr(), n, self.U8_LAYOUTS[layout]), "fpc_detect_u8")

    def detect_u8(self, frames_u8, layout):
        """frames_u8: uint8 [n,H,W] ("gray") or [n,H,W,3] ("rgb_hwc", "bgr_hwc", "bgr_hwc_gray")."""
        if not isinstance(frames_u8, torch.Tensor):
            frames_u8 = torch.from_numpy(np.ascontiguousarray(frames_u8, dtype=np.uint8))
        f = frames_u8.to(self.torch_device, torch.uint8).contiguous()
        want = (self.h, self.w) if layout == "gray" else (self.h, self.w, 3)
        if tuple(f.shape[1:]) != want or f.shape[0] > self.max_batch:
            raise ValueError("u8 frames must be [n<=%d,%s], got %s" % (self.max_batch, want, tuple(f.shape)))
        torch.cuda.synchronize(self.torch_device)
        self.detect_u8_async(f, f.shape[0], layout)
        return self.fetch(f.shape[0])

    def detect_u8_resized(self, frames_u8, layout="bgr_hwc"):
        """make_query_image (python/src/inference.py:72-85) + camera.py:31 on the device: uint8 [n,h,w,3] camera frames
        of any size -> resized to cover this engine's H x W, centre-cropped, converted, detected."""
        if not isinstance(frames_u8, torch.Tensor):
            frames_u8 = torch.from_numpy(np.ascontiguousarray(frames_u8, dtype=np.uint8))
        f = frames_u8.to(self.torch_device, torch.uint8).contiguous()
        if f.dim() != 4 or f.shape[3] != 3 or f.shape[0] > self.max_batch or layout not in ("rgb_hwc", "bgr_hwc"):
            raise ValueError("frames must be uint8 [n<=%d,h,w,3] in rgb_hwc / bgr_hwc layout" % self.max_batch)
        torch.cuda.synchronize(self.torch_device)
        _lib.check(self._l.fpc_detect_u8_resized(self._ctx, f.data_ptr(), f.shape[0], f.shape[1], f.shape[2],
                                                 self.U8_LAYOUTS[layout]), "fpc_detect_u8_resized")
        return self.fetch(f.shape[0])

    def u8_staging(self, n):
        """The float frames [n,C,H,W] the last detect_u8 call fed to the network (a copy)."""
        self.sync()
        ptr = self._l.fpc_u8_staging(self._ctx)
        nbytes = n * self.in_channels * self.h * self.w * 4
        raw = torch.as_tensor(_DevArray(ptr, nbytes), device=self.torch_device)   # uint8 view of the library's buffer
        return raw.view(torch.float32).reshape(n, self.in_channels, self.h, self.w).clone()

    def homography_adaptation(self, frames, homographies, inverses=None, erosion_radius=8, aggregation="sum"):
        """homography_adaptation (python/src/homographies.py:250-324): frames [n,C,H,W], homographies [num,8] (flat,
        the convention of sample_homography) -> aggregated probability maps [n,H,W] (CUDA tensor)."""
        frames = self._frames(frames)
        hs = np.ascontiguousarray(homographies, np.float32).reshape(-1, 8)
        inv = None if inverses is None else np.ascontiguousarray(inverses, np.float32).reshape(-1, 8)
        if inv is not None and inv.shape != hs.shape:
            raise ValueError("inverses must match homographies")
        if aggregation not in ("sum", "max"):
            raise ValueError("Unknown aggregation method: %s" % aggregation)        # homographies.py:322
        out = torch.empty((frames.shape[0], self.h, self.w), device=self.torch_device)
        torch.cuda.synchronize(self.torch_device)
        _lib.check(self._l.fpc_homography_adaptation(
            self._ctx, frames.data_ptr(), frames.shape[0], hs.ctypes.data, None if inv is None else inv.ctypes.data,
            hs.shape[0], int(erosion_radius), 1 if aggregation == "max" else 0, out.data_ptr()), "fpc_homography_adaptation")
        self.sync()
        return out

    def get_points(self, prob_map, desc_map=None):
        """Post-processing only, on caller-provided dense maps (netutils.py:78-121)."""
        prob_map = prob_map.to(self.torch_device, torch.float32).contiguous()
        n = prob_map.shape[0]
        dptr = None
        if desc_map is not None:
            desc_map = desc_map.to(self.torch_device, torch.float32).contiguous()
            dptr = desc_map.data_ptr()
        torch.cuda.synchronize(self.torch_device)
        _lib.check(self._l.fpc_get_points(self._ctx, prob_map.data_ptr(), dptr, n), "fpc_get_points")
        return self.fetch(n, with_desc=desc_map is not None)

    def sample_descriptors(self, desc_map, xy):
        """get_descriptors on its own (netutils.py:103-121): desc_map [D,H/8,W/8] (or [1,D,H/8,W/8]), xy float64 [K,2]
        (x, y) in pixels -> unit-norm descriptors float32 [K,D] (numpy)."""
        if not isinstance(desc_map, torch.Tensor):
            desc_map = torch.from_numpy(np.ascontiguousarray(desc_map, dtype=np.float32))
        dm = desc_map.to(self.torch_device, torch.float32).contiguous()
        if dm.dim() == 4 and dm.shape[0] == 1:
            dm = dm[0]
        if tuple(dm.shape) != (self.desc_dim, self.h // 8, self.w // 8):
            raise ValueError("descriptor map must be [%d,%d,%d], got %s" % (self.desc_dim, self.h // 8, self.w // 8, tuple(dm.shape)))
        pts = torch.from_numpy(np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)).to(self.torch_device)
        k = pts.shape[0]
        out = torch.empty((k, self.desc_dim), dtype=torch.float32, device=self.torch_device)
        torch.cuda.synchronize(self.torch_device)
        _lib.check(self._l.fpc_sample_descriptors(self._ctx, dm.data_ptr(), pts.data_ptr(), k, out.data_ptr()),
                   "fpc_sample_descriptors")
        self.sync()
        return out.cpu().numpy()

    ACTIVATIONS = ("pool", "layer1.0", "layer1.1", "layer2.0", "layer2.1", "det.0", "det.1", "desc_in.0", "desc_in.1",
                   "up", "desc_out.0", "desc_out.1")
    # arch="vgg" (superpoint::SPModel's modules): "det_b" is the logits, "desc_b" the descriptor map, L2-normalised
    VGG_ACTIVATIONS = ("conv0_a", "conv0_b", "pool0", "conv1_a", "conv1_b", "pool1", "conv2_a", "conv2_b", "pool2",
                       "conv3_a", "conv3_b", "det_a", "det_b", "desc_a", "desc_b")

    def activation(self, name, frame0=0, n=1):
        """Intermediate tensor of the LAST forward / detect call as a forward hook on the reference module would return
        it: float32 CUDA tensor [n,C,h,w] (fpc_read_activation).  "det.1" (the logits) raises after a `detect` in
        dtype="bf16" with the fused softmax epilogue -- that call never writes logits; `forward` always does.  An
        arch="vgg" engine takes the names of VGG_ACTIVATIONS instead (the desc_* ones raise with the descriptor head
        disabled)."""
        c, h, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(self._l.fpc_read_activation(self._ctx, name.encode(), frame0, n, None, ctypes.byref(c), ctypes.byref(h),
                                               ctypes.byref(w)), "fpc_read_activation")
        out = torch.empty((n, c.value, h.value, w.value), dtype=torch.float32, device=self.torch_device)
        torch.cuda.synchronize(self.torch_device)
        _lib.check(self._l.fpc_read_activation(self._ctx, name.encode(), frame0, n, out.data_ptr(), None, None, None),
                   "fpc_read_activation")
        self.sync()
        return out

    def sync(self):
        _lib.check(self._l.fpc_sync(self._ctx), "fpc_sync")

    def counts(self, n, allow_nonfinite=False):
        """fpc_get_counts.  A frame with a NaN / Inf pixel raises FpcError (code -9, FPC_E_NONFINITE) unless
        `allow_nonfinite`: the counts are delivered either way, and output_range() names the frame."""
        cnt = np.zeros(n, np.int32)
        ncand = np.zeros(n, np.int32)
        rc = self._l.fpc_get_counts(self._ctx, n, cnt.ctypes.data, ncand.ctypes.data)
        if not (allow_nonfinite and rc == -9):
            _lib.check(rc, "fpc_get_counts")
        return cnt, ncand

    def output_range(self, n):
        """fpc_output_range: per frame of the last call (max logit, max |descriptor map| (forward only), non-finite pixel?)."""
        ml, md, bad = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        _lib.check(self._l.fpc_output_range(self._ctx, n, ml.ctypes.data, md.ctypes.data, bad.ctypes.data), "fpc_output_range")
        return ml, md, bad.astype(bool)

    def fetch(self, n, with_desc=None, allow_nonfinite=False):
        """-> list of (xy int32[K,2], conf float32[K], desc float32[K,128] | None, n_candidates)."""
        if with_desc is None:
            with_desc = self.descriptor_enabled
        cnt, ncand = self.counts(n, allow_nonfinite)
        out = []
        for f in range(n):
            k = int(cnt[f])
            xy = np.empty((k, 2), np.int32)
            conf = np.empty(k, np.float32)
            desc = np.empty((k, self.desc_dim), np.float32) if with_desc else None
            got = self._l.fpc_get_keypoints(self._ctx, f, k, xy.ctypes.data, conf.ctypes.data,
                                            desc.ctypes.data if with_desc else None)
            _lib.check(got, "fpc_get_keypoints")
            assert got == k
            out.append((xy, conf, desc, int(ncand[f])))
        return out

    # -- descriptor matching (next row of the path) -------------------------------------
    def _desc(self, d):
        if not isinstance(d, torch.Tensor):
            d = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32))
        d = d.to(self.torch_device, torch.float32).contiguous()
        if d.dim() != 2 or d.shape[1] != self.desc_dim:
            raise ValueError("descriptors must be [n,%d]" % self.desc_dim)
        return d

    def match(self, query, train, cross_check=True, max_dist=0.0):
        """cv2.BFMatcher(NORM_L2, crossCheck).match(query, train): -> (match int32[nq] (train index or
        -1), dist float32[nq])."""
        q, t = self._desc(query), self._desc(train)
        m = torch.empty(q.shape[0], dtype=torch.int32, device=self.torch_device)
        d = torch.empty(q.shape[0], dtype=torch.float32, device=self.torch_device)
        torch.cuda.synchronize(self.torch_device)
        _lib.check(self._l.fpc_match(self._ctx, q.data_ptr(), q.shape[0], t.data_ptr(), t.shape[0],
                                     int(bool(cross_check)), float(max_dist), m.data_ptr(), d.data_ptr()), "fpc_match")
        self.sync()
        return m.cpu().numpy(), d.cpu().numpy()

    def first_within(self, key, cur, tolerance=0.8):
        """SearchKeyFrameCorrespondence (cpp/src/main.cc:18-29): first index in `cur` closer than tolerance."""
        k, c = self._desc(key), self._desc(cur)
        out = torch.empty(k.shape[0], dtype=torch.int32, device=self.torch_device)
        torch.cuda.synchronize(self.torch_device)
        _lib.check(self._l.fpc_first_within(self._ctx, k.data_ptr(), k.shape[0], c.data_ptr(), c.shape[0],
                                            float(tolerance), out.data_ptr()), "fpc_first_within")
        self.sync()
        return out.cpu().numpy()

    # -- the same rules over the last detect's batch, on the device (fpc_match_frames / fpc_first_within_frames) ----
    PAIRINGS = {"key": 0, "previous": 1}     # FPC_PAIR_KEY / FPC_PAIR_PREVIOUS (include/fpc.h)

    def _results_view(self):
        """(desc [B,cap,D], count [B]) aliasing the library's device results (fpc_results)."""
        cap, dd, b = self.capacity, self.desc_dim, self.max_batch
        desc = torch.as_tensor(_DevArray(self._res.desc, b * cap * dd * 4), device=self.torch_device)
        count = torch.as_tensor(_DevArray(self._res.count, b * 4), device=self.torch_device)
        return desc.view(torch.float32).view(b, cap, dd), count.view(torch.int32)

    def keep_frame(self, f):
        """A device copy of frame f's descriptors [cap,D] and of its device count [1] (int32), ordered on the ctx stream
        behind the last detect: the next call's key, with no host round trip."""
        if not self.descriptor_enabled or not 0 <= f < self.max_batch:
            raise ValueError("keep_frame needs descriptors and 0 <= f < max_batch")
        desc, count = self._results_view()
        with torch.cuda.stream(self.torch_stream()):
            return desc[f].clone(), count[f:f + 1].clone()

    def _key(self, key):
        """key -> (descriptors, device count) on the device, or (None, None).  A (desc, count) pair (keep_frame) is
        used as it is; a host array or tensor [k,D] is uploaded together with a device count k."""
        if key is None:
            return None, None
        if isinstance(key, tuple):
            d, c = key
            if d.device != self.torch_device or d.dtype != torch.float32 or d.dim() != 2 or d.shape[1] != self.desc_dim \
                    or c.device != self.torch_device or c.dtype != torch.int32:
                raise ValueError("a (desc, count) key must be device tensors float32 [k,%d] and int32 [1]" % self.desc_dim)
            return d.contiguous(), c
        d = self._desc(key)
        return d, torch.tensor([d.shape[0]], dtype=torch.int32, device=self.torch_device)

    def _enqueue(self, call):
        """Runs `call` on the ctx stream ordered after the caller's current torch stream (and the caller's stream after
        it): GPU-side waits only, no host synchronisation."""
        cur, st = torch.cuda.current_stream(self.torch_device), self.torch_stream()
        st.wait_stream(cur)
        call()
        cur.wait_stream(st)

    # -- what the wrappers below are made of ----------------------------------------------------------------------------
    def _call(self, name, *args, inputs=()):
        """fpc_<name>(ctx, *args) through _enqueue, tensors passed as their device pointers.  `inputs`: the caller's tensors
        the call reads (entries that are no tensor are skipped) -- the caching allocator must not hand their memory out
        before the ctx stream read it."""
        fn = getattr(self._l, name)
        self._enqueue(lambda: _lib.check(fn(self._ctx, *(_ptr(a) for a in args)), name))
        for t in inputs:
            if isinstance(t, torch.Tensor):
                t.record_stream(self.torch_stream())

    def _int32(self, *shape):
        return torch.empty(shape, dtype=torch.int32, device=self.torch_device)

    def _table(self, *lead):
        """An empty (match int32, dist float32) table pair [*lead, cap]."""
        return self._int32(*lead, self.capacity), torch.empty((*lead, self.capacity), dtype=torch.float32,
                                                              device=self.torch_device)

    def _ransac_out(self, *lead, stride=None):
        """Empty RANSAC outputs (H float32 [*lead,3,3], ninliers int32 [*lead], mask uint8 [*lead,stride or cap])."""
        return (torch.empty((*lead, 3, 3), dtype=torch.float32, device=self.torch_device), self._int32(*lead),
                torch.empty((*lead, self.capacity if stride is None else stride), dtype=torch.uint8, device=self.torch_device))

    def _dev_int32(self, name, t, text, *shape):
        """`t`, contiguous, if it is an int32 tensor of `shape` (None: any extent) on this device; `text` is the shape as
        the error names it."""
        if t.device != self.torch_device or t.dtype != torch.int32 or t.dim() != len(shape) \
                or any(w is not None and s != w for s, w in zip(t.shape, shape)):
            raise ValueError("%s must be a device tensor int32 %s" % (name, text))
        return t.contiguous()

    def _pairing(self, pairing):
        if pairing not in self.PAIRINGS:
            raise ValueError("pairing must be one of %s, got %r" % (sorted(self.PAIRINGS), pairing))
        return self.PAIRINGS[pairing]

    def _frame_counts(self, n):
        return self._results_view()[1][:n].cpu().numpy()

    def _host(self, tensors):
        self.sync()
        return tuple(None if t is None else t.cpu().numpy() for t in tensors)

    def _dev_uint8(self, t):
        """A bool / integer mask (device tensor or host array) as a contiguous uint8 device tensor."""
        t = torch.as_tensor(t).to(self.torch_device)
        return (t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)).contiguous()

    def _per_frame(self, n, m, d):
        m, d = self._host((m, d))
        cnt = self._frame_counts(n)
        return [(m[f, :cnt[f]].copy(), d[f, :cnt[f]].copy()) for f in range(n)]

    def match_frames_async(self, n, key=None, pairing="key", cross_check=True, max_dist=0.0, ratio=0.0):
        """fpc_match_frames: every frame of the last detect against the key set ("key") or its predecessor in the batch
        ("previous"; frame 0 against the key, or nothing without one) -> (match int32 [n,cap], dist float32 [n,cap]) on
        the device; rows past a frame's count are -1.  Does not synchronise."""
        pair = self._pairing(pairing)
        kd, kc = self._key(key)
        m, d = self._table(n)
        self._call("fpc_match_frames", n, pair, kd, kc, int(bool(cross_check)), float(max_dist), float(ratio), m, d,
                   inputs=(kd, kc))
        return m, d

    def match_frames(self, n, key=None, pairing="key", cross_check=True, max_dist=0.0, ratio=0.0):
        """match_frames_async, then per frame (match int32 [K_f], dist float32 [K_f])."""
        return self._per_frame(n, *self.match_frames_async(n, key, pairing, cross_check, max_dist, ratio))

    def first_within_frames_async(self, n, key, tolerance=0.8):
        """fpc_first_within_frames -> int32 [n,cap] on the device: per key row, the first row of frame f closer than
        `tolerance`, or -1 (rows past the key's count: -1).  Does not synchronise."""
        kd, kc = self._key(key)
        if kd is None:
            raise ValueError("first_within_frames needs a key set")
        out = self._int32(n, self.capacity)
        self._call("fpc_first_within_frames", n, kd, kc, float(tolerance), out, inputs=(kd, kc))
        return out, kc

    def first_within_frames(self, n, key, tolerance=0.8):
        """SearchKeyFrameCorrespondence for every frame of the last detect: per frame int32 [nkey]."""
        out, kc = self.first_within_frames_async(n, key, tolerance)
        out, kc = self._host((out, kc))
        nk = min(max(int(kc[0]), 0), self.capacity)
        return [out[f, :nk].copy() for f in range(n)]

    # -- geometric verification: RANSAC homographies on the device (fpc_ransac_homography / fpc_homography_frames) -----
    def _points_view(self):
        """(xy [B,cap,2] int32, count [B] int32) aliasing the library's device results (fpc_results)."""
        cap, b = self.capacity, self.max_batch
        xy = torch.as_tensor(_DevArray(self._res.xy, b * cap * 2 * 4), device=self.torch_device)
        count = torch.as_tensor(_DevArray(self._res.count, b * 4), device=self.torch_device)
        return xy.view(torch.int32).view(b, cap, 2), count.view(torch.int32)

    def keep_frame_points(self, f):
        """A device copy of frame f's keypoint coordinates xy [cap,2] (int32), ordered on the ctx stream behind the last
        detect: keep_frame's companion, the key_xy of homography_frames (rows past the frame's count are never referenced
        by a match table made against keep_frame(f))."""
        if not 0 <= f < self.max_batch:
            raise ValueError("keep_frame_points needs 0 <= f < max_batch")
        with torch.cuda.stream(self.torch_stream()):
            return self._points_view()[0][f].clone()

    # -- what the geometry wrappers are made of: a parameter struct, one of three pair sources, a solver call ----------------
    _RANSAC_FIELDS = ("iterations", "reproj_threshold", "seed", "refits", "min_inliers")

    def _params(self, struct, default, fields, word, params):
        """A `struct` filled by fpc_<default> and then from `params`, whose keys must be among `fields`; `word` names the
        family in the TypeError."""
        p = struct()
        _lib.check(getattr(self._l, default)(ctypes.byref(p)), default)
        for k, v in params.items():
            if k not in fields:
                raise TypeError("unknown %s parameter %r" % (word, k))
            setattr(p, k, v)
        return p

    def _ransac_params(self, params):
        return self._params(_lib.FpcRansacParams, "fpc_default_ransac_params", self._RANSAC_FIELDS, "RANSAC", params)

    def _explicit_pairs(self, a, b, npairs, width=2, text="src and dst must be [n,stride,2] and npairs [n]", first=2):
        """Explicit pairs on the device: a float32 [n,stride,first], b float32 [n,stride,width], npairs int32 [n] -> (n, the
        calls' arguments (a, b, npairs, stride))."""
        a = torch.as_tensor(a).to(self.torch_device, torch.float32).contiguous()
        b = torch.as_tensor(b).to(self.torch_device, torch.float32).contiguous()
        npairs = torch.as_tensor(npairs).to(self.torch_device, torch.int32).contiguous()
        if a.dim() != 3 or a.shape[2] != first or b.shape != (*a.shape[:2], width) or npairs.shape != (a.shape[0],):
            raise ValueError(text)
        return int(a.shape[0]), (a, b, npairs, int(a.shape[1]))

    def _frames_pairs(self, n, pairing, key_xy, match, fill, *args):
        """The frames' pair source -> (fill(*args), the calls' arguments (pairing, key_xy, its device count, match)).
        `fill` makes the call's parameter struct, between the pairing's check and the key's as it always was."""
        pair = self._pairing(pairing)
        p = fill(*args)
        kx, kc = self._key_xy(key_xy)
        return p, (pair, kx, kc, self._dev_int32("match", match, "[n,%d]" % self.capacity, n, self.capacity))

    def _bank_pairs(self, n, slot, match, fill, *args):
        """The bank's pair source -> (fill(*args), the calls' arguments (slot, match)); `fill` as in _frames_pairs, behind
        the check that a bank exists."""
        self._bank_info()
        p = fill(*args)
        slot = self._dev_int32("slot", slot, "[n]", n)
        return p, (slot, self._dev_int32("match", match, "[n,%d]" % self.capacity, n, self.capacity))

    def _solve(self, name, n, pairs, p, out, *more, tail=()):
        """fpc_<name>(ctx, n, *pairs, *more, params, *out, *tail) -> out, its last tensor (a uint8 mask, or None) as bool,
        then the tensors of `tail` as they are."""
        self._call(name, n, *pairs, *more, ctypes.byref(p), *out, *tail, inputs=(*pairs, *more))
        return (*out[:-1], None if out[-1] is None else out[-1].view(torch.bool), *tail)

    def _key_xy(self, key_xy):
        """key_xy -> (xy int32 [k,2], device count) or (None, None).  An (xy, count) pair of device tensors is used as it
        is; a device tensor or host array [k,2] gets the device count k."""
        if key_xy is None:
            return None, None
        if isinstance(key_xy, tuple):
            xy, c = key_xy
            if xy.device != self.torch_device or xy.dtype != torch.int32 or xy.dim() != 2 or xy.shape[1] != 2 \
                    or c.device != self.torch_device or c.dtype != torch.int32:
                raise ValueError("an (xy, count) key must be device tensors int32 [k,2] and int32 [1]")
            return xy.contiguous(), c
        xy = key_xy if isinstance(key_xy, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(key_xy, dtype=np.int32))
        xy = xy.to(self.torch_device, torch.int32).contiguous()
        if xy.dim() != 2 or xy.shape[1] != 2:
            raise ValueError("key_xy must be [k,2]")
        return xy, torch.tensor([xy.shape[0]], dtype=torch.int32, device=self.torch_device)

    def ransac_homography_async(self, src, dst, npairs, **params):
        """fpc_ransac_homography: src / dst float32 [n,stride,2] and npairs int32 [n] (device tensors or host arrays) ->
        device tensors (H float32 [n,3,3] mapping src to dst with H[2,2] = 1, ninliers int32 [n], inlier bool [n,stride]);
        a failed frame has H = 0 and no inliers.  Parameters: the fields of fpc_ransac_params.  Does not synchronise."""
        p = self._ransac_params(params)
        n, pairs = self._explicit_pairs(src, dst, npairs)
        return self._solve("fpc_ransac_homography", n, pairs, p, self._ransac_out(n, stride=pairs[3]))

    def ransac_homography(self, src, dst, npairs, **params):
        """ransac_homography_async, then host arrays (H [n,3,3], ninliers [n], inlier bool [n,stride])."""
        return self._host(self.ransac_homography_async(src, dst, npairs, **params))

    def homography_frames_async(self, n, match, key_xy=None, pairing="key", **params):
        """fpc_homography_frames: the pairs (xy[f][i], train_xy[match[f][i]]) of every frame of the last detect, `match`
        being match_frames_async's table (int32 [n,cap], device) for the same pairing and key, `key_xy` the key frame's
        coordinates (keep_frame_points) -> device tensors (H [n,3,3], ninliers [n], inlier bool [n,cap] by query row).
        Does not synchronise."""
        p, pairs = self._frames_pairs(n, pairing, key_xy, match, self._ransac_params, params)
        return self._solve("fpc_homography_frames", n, pairs, p, self._ransac_out(n))

    def homography_frames(self, n, match, key_xy=None, pairing="key", **params):
        """homography_frames_async, then host arrays (H [n,3,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.homography_frames_async(n, match, key_xy, pairing, **params))

    # -- key-frame bank: a batch against many stored key frames (fpc_bank_* / fpc_match_bank / fpc_homography_bank) -----
    BANK_FORMATS = {"f32": 0, "bf16": 1}          # include/fpc.h FPC_BANK_F32 / FPC_BANK_BF16

    def bank_create(self, slots, rows=None, format="f32"):
        """fpc_bank_create_ex: a device-resident bank of `slots` key frames of up to `rows` keypoints each (default: the
        capacity).  format "bf16" stores the rows in bf16 and matches on the bf16 matrix path: half the memory per frame,
        distances within the rounding of the rows instead of fpc_match_frames' bits (include/fpc.h).  The only bank call
        that allocates; one bank per engine."""
        if format not in self.BANK_FORMATS:
            raise ValueError("format must be one of %s, got %r" % (sorted(self.BANK_FORMATS), format))
        _lib.check(self._l.fpc_bank_create_ex(self._ctx, int(slots), int(self.capacity if rows is None else rows),
                                              self.BANK_FORMATS[format]), "fpc_bank_create_ex")
        v = _lib.FpcBankView()
        _lib.check(self._l.fpc_bank_get(self._ctx, ctypes.byref(v)), "fpc_bank_get")
        fmt, ptr = ctypes.c_int(-1), ctypes.c_void_p()
        _lib.check(self._l.fpc_bank_format(self._ctx, ctypes.byref(fmt), ctypes.byref(ptr)), "fpc_bank_format")
        self._bank = v
        self._bank_format = (format, ptr.value)
        return v.bytes

    def bank_destroy(self):
        _lib.check(self._l.fpc_bank_destroy(self._ctx), "fpc_bank_destroy")
        self._bank = None

    def _bank_info(self):
        v = getattr(self, "_bank", None)
        if v is None:
            raise ValueError("the engine has no key-frame bank (bank_create)")
        return v

    def bank_view(self):
        """(desc float32 [slots,rows,D] -- bfloat16 for a "bf16" bank --, xy int32 [slots,rows,2], count int32 [slots])
        aliasing the bank's device memory (fpc_bank_get / fpc_bank_format); `bank_info()` has the sizes."""
        v = self._bank_info()
        s, r, dd = v.slots, v.rows, v.desc_dim
        fmt, ptr = self._bank_format
        elem, dtype = (2, torch.bfloat16) if fmt == "bf16" else (4, torch.float32)
        desc = torch.as_tensor(_DevArray(ptr, s * r * dd * elem), device=self.torch_device)
        xy = torch.as_tensor(_DevArray(v.xy, s * r * 2 * 4), device=self.torch_device)
        count = torch.as_tensor(_DevArray(v.count, s * 4), device=self.torch_device)
        return desc.view(dtype).view(s, r, dd), xy.view(torch.int32).view(s, r, 2), count.view(torch.int32)

    def bank_info(self):
        """{"slots", "rows", "desc_dim", "chunk" (slots scored per pass), "bytes" (allocated, workspace included),
        "format" ("f32" / "bf16")}."""
        v = self._bank_info()
        return {"slots": v.slots, "rows": v.rows, "desc_dim": v.desc_dim, "chunk": v.chunk, "bytes": v.bytes,
                "format": self._bank_format[0]}

    def bank_store(self, frame, slot):
        """fpc_bank_store: frame `frame` of the last detect into slot `slot` (its most confident `rows` keypoints), on the
        ctx stream behind that detect.  Does not synchronise."""
        self._call("fpc_bank_store", int(frame), int(slot))

    def bank_store_rows(self, slot, desc, xy):
        """fpc_bank_store_rows: a saved key frame into slot `slot`: desc [k,D], xy [k,2] (host arrays or device tensors),
        or device pairs (desc, count) / (xy, count) as keep_frame / keep_frame_points make them.  Does not synchronise."""
        d, n = self._key(desc)
        x, _ = self._key_xy(xy)
        if d is None or x is None or x.shape[0] < d.shape[0]:
            raise ValueError("bank_store_rows needs descriptors [k,D] and coordinates [k,2]")
        self._call("fpc_bank_store_rows", int(slot), d, x, n, inputs=(d, x, n))

    def bank_clear(self, slot=None):
        """fpc_bank_clear: empties slot `slot`, or every slot."""
        s = -1 if slot is None else int(slot)
        if s < 0 and slot is not None:
            raise ValueError("slot must be >= 0 (None clears every slot)")
        self._call("fpc_bank_clear", s)

    def match_bank_async(self, n, cross_check=True, max_dist=0.0, ratio=0.0, min_score=0, table=True):
        """fpc_match_bank: every frame of the last detect against every slot of the bank -> device tensors (score int32
        [n,slots], best int32 [n] (-1: no slot reached max(min_score, 1)), match int32 [n,cap], dist float32 [n,cap]) --
        the last two are match_frames_async's table against slot best[f] (None with table=False).  Give max_dist or
        ratio: a bare cross check does not tell slots apart (include/fpc.h).  Does not synchronise."""
        score, best = self._int32(n, self._bank_info().slots), self._int32(n)
        m, d = self._table(n) if table else (None, None)
        self._call("fpc_match_bank", n, int(bool(cross_check)), float(max_dist), float(ratio), int(min_score), score, best,
                   m, d)
        return score, best, m, d

    def match_bank(self, n, cross_check=True, max_dist=0.0, ratio=0.0, min_score=0):
        """match_bank_async, then host arrays: (score [n,slots], best [n], [(match int32 [K_f], dist float32 [K_f])])."""
        score, best, m, d = self.match_bank_async(n, cross_check, max_dist, ratio, min_score)
        tables = self._per_frame(n, m, d)
        return score.cpu().numpy(), best.cpu().numpy(), tables

    def homography_bank_async(self, n, slot, match, **params):
        """fpc_homography_bank: homography_frames_async with frame f's key coordinates taken from bank slot slot[f] (int32
        [n], device; normally match_bank_async's `best`) and `match` that call's table -> device tensors (H [n,3,3],
        ninliers [n], inlier bool [n,cap]); a frame with slot -1 fails (H = 0).  Does not synchronise."""
        p, pairs = self._bank_pairs(n, slot, match, self._ransac_params, params)
        return self._solve("fpc_homography_bank", n, pairs, p, self._ransac_out(n))

    def homography_bank(self, n, slot, match, **params):
        """homography_bank_async, then host arrays (H [n,3,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.homography_bank_async(n, slot, match, **params))

    # -- epipolar verification: RANSAC fundamental matrices (fpc_ransac_fundamental / fpc_fundamental_frames / _bank) --------
    def ransac_fundamental_async(self, src, dst, npairs, **params):
        """fpc_ransac_fundamental: ransac_homography_async's arguments -> device tensors (F float32 [n,3,3] with
        (u, v, 1) F (x, y, 1)^T = 0 for a src pixel (x, y) and its dst pixel (u, v), norm 1, rank 2; ninliers int32 [n];
        inlier bool [n,stride], the pairs within reproj_threshold in Sampson distance); a failed frame has F = 0 and no
        inliers.  min_inliers must be >= 8.  Does not synchronise."""
        p = self._ransac_params(params)
        n, pairs = self._explicit_pairs(src, dst, npairs)
        return self._solve("fpc_ransac_fundamental", n, pairs, p, self._ransac_out(n, stride=pairs[3]))

    def ransac_fundamental(self, src, dst, npairs, **params):
        """ransac_fundamental_async, then host arrays (F [n,3,3], ninliers [n], inlier bool [n,stride])."""
        return self._host(self.ransac_fundamental_async(src, dst, npairs, **params))

    def fundamental_frames_async(self, n, match, key_xy=None, pairing="key", **params):
        """fpc_fundamental_frames: homography_frames_async's arguments and pairs -> device tensors (F [n,3,3], ninliers
        [n], inlier bool [n,cap] by query row).  Does not synchronise."""
        p, pairs = self._frames_pairs(n, pairing, key_xy, match, self._ransac_params, params)
        return self._solve("fpc_fundamental_frames", n, pairs, p, self._ransac_out(n))

    def fundamental_frames(self, n, match, key_xy=None, pairing="key", **params):
        """fundamental_frames_async, then host arrays (F [n,3,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.fundamental_frames_async(n, match, key_xy, pairing, **params))

    def fundamental_bank_async(self, n, slot, match, **params):
        """fpc_fundamental_bank: fundamental_frames_async with frame f's key coordinates taken from bank slot slot[f], as
        homography_bank_async -> device tensors (F [n,3,3], ninliers [n], inlier bool [n,cap]); a frame with slot -1
        fails (F = 0).  Does not synchronise."""
        p, pairs = self._bank_pairs(n, slot, match, self._ransac_params, params)
        return self._solve("fpc_fundamental_bank", n, pairs, p, self._ransac_out(n))

    def fundamental_bank(self, n, slot, match, **params):
        """fundamental_bank_async, then host arrays (F [n,3,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.fundamental_bank_async(n, slot, match, **params))

    # -- minimal-sample relative pose: RANSAC essential matrices, 5 + 1 pairs (fpc_ransac_essential / _frames / _bank) ------
    def _essential_params(self, K_query, K_train, params):
        return self._two_camera_params(_lib.FpcEssentialParams, "fpc_default_essential_params", self._RANSAC_FIELDS,
                                       "essential", K_query, K_train, params)

    def _essential_out(self, n, stride=None):
        """Empty outputs (F float32 [n,3,3], E float32 [n,3,3], ninliers int32 [n], mask uint8 [n,stride or cap])."""
        f, ninl, mask = self._ransac_out(n, stride=stride)
        return f, torch.empty_like(f), ninl, mask

    def ransac_essential_async(self, src, dst, npairs, K_query=None, K_train=None, **params):
        """fpc_ransac_essential: ransac_fundamental_async's pairs and the two cameras (3 x 3 matrices or (fx, fy, cx, cy))
        -> device tensors (F float32 [n,3,3] in ransac_fundamental_async's form, which pose_*, refine_pose_* and the
        epipolar guided matchers take as it is; E float32 [n,3,3], the same matrix in normalised coordinates, norm 1;
        ninliers int32 [n]; inlier bool [n,stride]).  A sample is 5 + 1 pairs, so planar scenes are solved and far fewer
        iterations are needed than by the 8-point; an exactly planar scene has two valid answers, one is returned.  A failed
        frame is all zeros.  min_inliers must be >= 6.  Does not synchronise."""
        p = self._essential_params(K_query, K_train, params)
        n, pairs = self._explicit_pairs(src, dst, npairs)
        return self._solve("fpc_ransac_essential", n, pairs, p, self._essential_out(n, stride=pairs[3]))

    def ransac_essential(self, src, dst, npairs, K_query=None, K_train=None, **params):
        """ransac_essential_async, then host arrays (F [n,3,3], E [n,3,3], ninliers [n], inlier bool [n,stride])."""
        return self._host(self.ransac_essential_async(src, dst, npairs, K_query, K_train, **params))

    def essential_frames_async(self, n, match, key_xy=None, pairing="key", K_query=None, K_train=None, **params):
        """fpc_essential_frames: fundamental_frames_async's arguments and pairs -> device tensors (F [n,3,3], E [n,3,3],
        ninliers [n], inlier bool [n,cap] by query row).  Does not synchronise."""
        p, pairs = self._frames_pairs(n, pairing, key_xy, match, self._essential_params, K_query, K_train, params)
        return self._solve("fpc_essential_frames", n, pairs, p, self._essential_out(n))

    def essential_frames(self, n, match, key_xy=None, pairing="key", K_query=None, K_train=None, **params):
        """essential_frames_async, then host arrays (F [n,3,3], E [n,3,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.essential_frames_async(n, match, key_xy, pairing, K_query, K_train, **params))

    def essential_bank_async(self, n, slot, match, K_query=None, K_train=None, **params):
        """fpc_essential_bank: essential_frames_async with frame f's key coordinates taken from bank slot slot[f], as
        fundamental_bank_async -> device tensors (F [n,3,3], E [n,3,3], ninliers [n], inlier bool [n,cap]); a frame with
        slot -1 fails (zeros).  Does not synchronise."""
        p, pairs = self._bank_pairs(n, slot, match, self._essential_params, K_query, K_train, params)
        return self._solve("fpc_essential_bank", n, pairs, p, self._essential_out(n))

    def essential_bank(self, n, slot, match, K_query=None, K_train=None, **params):
        """essential_bank_async, then host arrays (F [n,3,3], E [n,3,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.essential_bank_async(n, slot, match, K_query, K_train, **params))

    # -- relative pose from the fundamental matrices: R, t and triangulated points (fpc_pose_fundamental / _frames / _bank) ---
    @staticmethod
    def _intrinsics(k, name):
        """A 3 x 3 camera matrix or (fx, fy, cx, cy) -> (fx, fy, cx, cy); None: the defaults of fpc_default_pose_params."""
        if k is None:
            return None
        k = np.asarray(k, dtype=np.float64)
        if k.shape == (3, 3):
            if k[0, 1] != 0 or k[1, 0] != 0 or k[2, 0] != 0 or k[2, 1] != 0 or k[2, 2] != 1:
                raise ValueError("%s must be [fx 0 cx; 0 fy cy; 0 0 1]" % name)
            return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
        if k.shape == (4,):
            return tuple(float(v) for v in k)
        raise ValueError("%s must be a 3 x 3 matrix or (fx, fy, cx, cy)" % name)

    def _two_camera_params(self, struct, default, fields, word, K_query, K_train, params):
        """_params for a struct that starts with the query and the train camera (q_fx .. t_cy)."""
        cameras = (("q", self._intrinsics(K_query, "K_query")), ("t", self._intrinsics(K_train, "K_train")))
        p = self._params(struct, default, fields, word, params)
        for side, k in cameras:
            if k is not None:
                for field, v in zip(("fx", "fy", "cx", "cy"), k):
                    setattr(p, "%s_%s" % (side, field), v)
        return p

    def _pose_params(self, K_query, K_train, params):
        return self._two_camera_params(_lib.FpcPoseParams, "fpc_default_pose_params", ("reproj_threshold", "min_front"),
                                       "pose", K_query, K_train, params)

    def _pose_out(self, n, stride, points):
        """Empty pose outputs (R float32 [n,3,3], t float32 [n,3], nfront int32 [n], xyz float32 [n,stride,3], front uint8
        [n,stride]); the last two None without `points`."""
        dev = self.torch_device
        rm, tv = torch.empty((n, 3, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
        xyz = torch.empty((n, stride, 3), dtype=torch.float32, device=dev) if points else None
        front = torch.empty((n, stride), dtype=torch.uint8, device=dev) if points else None
        return rm, tv, self._int32(n), xyz, front

    def _pose(self, name, n, pairs, F, p, stride, points):
        """fpc_<name> behind its pair source: F [n,3,3] goes in front of the parameters."""
        return self._solve(name, n, pairs, p, self._pose_out(n, stride, points), self._guided_h(n, F, "F"))

    def pose_fundamental_async(self, src, dst, npairs, F, K_query=None, K_train=None, points=True, **params):
        """fpc_pose_fundamental: ransac_fundamental_async's pairs and the F it returned (device [n,3,3] as it is, or a host
        array) -> device tensors (R float32 [n,3,3] and t float32 [n,3] with X_train = R X_query + t, |t| = 1; nfront int32
        [n]; xyz float32 [n,stride,3], the triangulated points in the query camera's frame; front bool [n,stride], the
        pairs in front of both cameras); xyz and front are None with points=False.  K_query / K_train: 3 x 3 camera
        matrices or (fx, fy, cx, cy).  Parameters: reproj_threshold, min_front.  A failed frame is all zeros.  Does not
        synchronise."""
        p = self._pose_params(K_query, K_train, params)
        n, pairs = self._explicit_pairs(src, dst, npairs)
        return self._pose("fpc_pose_fundamental", n, pairs, F, p, pairs[3], points)

    def pose_fundamental(self, src, dst, npairs, F, K_query=None, K_train=None, points=True, **params):
        """pose_fundamental_async, then host arrays (R [n,3,3], t [n,3], nfront [n], xyz [n,stride,3], front bool
        [n,stride])."""
        return self._host(self.pose_fundamental_async(src, dst, npairs, F, K_query, K_train, points, **params))

    def pose_frames_async(self, n, match, F, key_xy=None, pairing="key", K_query=None, K_train=None, points=True, **params):
        """fpc_pose_frames: fundamental_frames_async's arguments, pairs and output F -> device tensors (R [n,3,3], t [n,3],
        nfront [n], xyz [n,cap,3] and front bool [n,cap] by query row).  Does not synchronise."""
        p, pairs = self._frames_pairs(n, pairing, key_xy, match, self._pose_params, K_query, K_train, params)
        return self._pose("fpc_pose_frames", n, pairs, F, p, self.capacity, points)

    def pose_frames(self, n, match, F, key_xy=None, pairing="key", K_query=None, K_train=None, points=True, **params):
        """pose_frames_async, then host arrays (R [n,3,3], t [n,3], nfront [n], xyz [n,cap,3], front bool [n,cap])."""
        return self._host(self.pose_frames_async(n, match, F, key_xy, pairing, K_query, K_train, points, **params))

    def pose_bank_async(self, n, slot, match, F, K_query=None, K_train=None, points=True, **params):
        """fpc_pose_bank: pose_frames_async with frame f's key coordinates taken from bank slot slot[f], as
        fundamental_bank_async, and F that call's output; a frame with slot -1 fails (zeros).  Does not synchronise."""
        p, pairs = self._bank_pairs(n, slot, match, self._pose_params, K_query, K_train, params)
        return self._pose("fpc_pose_bank", n, pairs, F, p, self.capacity, points)

    def pose_bank(self, n, slot, match, F, K_query=None, K_train=None, points=True, **params):
        """pose_bank_async, then host arrays (R [n,3,3], t [n,3], nfront [n], xyz [n,cap,3], front bool [n,cap])."""
        return self._host(self.pose_bank_async(n, slot, match, F, K_query, K_train, points, **params))

    # -- relative pose from the homographies: planar scenes and pure rotations (fpc_pose_homography / _frames / _bank) ---------
    POSE_H_KINDS = {"failed": 0, "unique": 1, "twofold": 2, "rotation": 3}       # include/fpc.h FPC_POSE_H_*

    def _pose_h_params(self, K_query, K_train, params):
        return self._two_camera_params(_lib.FpcPoseHomographyParams, "fpc_default_pose_homography_params",
                                       ("reproj_threshold", "min_front", "min_baseline", "which"), "homography pose",
                                       K_query, K_train, params)

    def _pose_h_out(self, n, stride, points):
        """Empty outputs (kind int32 [n], R float32 [n,2,3,3], t float32 [n,2,3], plane float32 [n,2,4], nfront int32 [n,2],
        nplane int32 [n,2], xyz float32 [n,stride,3], front uint8 [n,stride]); the last two None without `points`."""
        dev = self.torch_device
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        xyz = f32(n, stride, 3) if points else None
        front = torch.empty((n, stride), dtype=torch.uint8, device=dev) if points else None
        return i32(n), f32(n, 2, 3, 3), f32(n, 2, 3), f32(n, 2, 4), i32(n, 2), i32(n, 2), xyz, front

    def _pose_h(self, name, n, pairs, H, p, stride, points):
        """fpc_<name> behind its pair source: H [n,3,3] goes in front of the parameters."""
        return self._solve(name, n, pairs, p, self._pose_h_out(n, stride, points), self._guided_h(n, H, "H"))

    def pose_homography_async(self, src, dst, npairs, H, K_query=None, K_train=None, points=True, **params):
        """fpc_pose_homography: ransac_homography_async's pairs and the H it returned (device [n,3,3] as it is, or a host
        array) -> device tensors (kind int32 [n], see POSE_H_KINDS; R float32 [n,2,3,3] and t float32 [n,2,3] of solutions 0
        and 1 with X_train = R X_query + t, |t| = 1; plane float32 [n,2,4], (N, d) with N.X = d in the query camera's
        frame; nfront int32 [n,2], the support; nplane int32 [n,2], the plane pairs in front; xyz float32 [n,stride,3]
        and front bool [n,stride], the points of solution `which`); xyz and front are None with points=False.  K_query /
        K_train: 3 x 3 camera matrices or (fx, fy, cx, cy).  Parameters: reproj_threshold, min_front, min_baseline,
        which.  A solution that does not exist is all zeros; a pure rotation has solution 0's R and nothing else.  Does
        not synchronise."""
        p = self._pose_h_params(K_query, K_train, params)
        n, pairs = self._explicit_pairs(src, dst, npairs)
        return self._pose_h("fpc_pose_homography", n, pairs, H, p, pairs[3], points)

    def pose_homography(self, src, dst, npairs, H, K_query=None, K_train=None, points=True, **params):
        """pose_homography_async, then host arrays."""
        return self._host(self.pose_homography_async(src, dst, npairs, H, K_query, K_train, points, **params))

    def pose_homography_frames_async(self, n, match, H, key_xy=None, pairing="key", K_query=None, K_train=None, points=True,
                                     **params):
        """fpc_pose_homography_frames: homography_frames_async's arguments, pairs and output H -> pose_homography_async's
        tensors with xyz [n,cap,3] and front bool [n,cap] by query row.  Does not synchronise."""
        p, pairs = self._frames_pairs(n, pairing, key_xy, match, self._pose_h_params, K_query, K_train, params)
        return self._pose_h("fpc_pose_homography_frames", n, pairs, H, p, self.capacity, points)

    def pose_homography_frames(self, n, match, H, key_xy=None, pairing="key", K_query=None, K_train=None, points=True,
                               **params):
        """pose_homography_frames_async, then host arrays."""
        return self._host(self.pose_homography_frames_async(n, match, H, key_xy, pairing, K_query, K_train, points, **params))

    def pose_homography_bank_async(self, n, slot, match, H, K_query=None, K_train=None, points=True, **params):
        """fpc_pose_homography_bank: pose_homography_frames_async with frame f's key coordinates taken from bank slot
        slot[f], as homography_bank_async, and H that call's output; a frame with slot -1 fails (zeros).  xyz[f] and
        front[f] go into bank_store_landmarks as they are.  Does not synchronise."""
        p, pairs = self._bank_pairs(n, slot, match, self._pose_h_params, K_query, K_train, params)
        return self._pose_h("fpc_pose_homography_bank", n, pairs, H, p, self.capacity, points)

    def pose_homography_bank(self, n, slot, match, H, K_query=None, K_train=None, points=True, **params):
        """pose_homography_bank_async, then host arrays."""
        return self._host(self.pose_homography_bank_async(n, slot, match, H, K_query, K_train, points, **params))

    # -- two-view bundle adjustment of a pose call's R, t and points (fpc_refine_pose / _frames / _bank) -------------------------
    def _refine_params(self, K_query, K_train, params):
        return self._two_camera_params(_lib.FpcRefineParams, "fpc_default_refine_params",
                                       ("reproj_threshold", "min_parallax_deg", "iterations", "lambda0", "min_front"),
                                       "refine", K_query, K_train, params)

    def _refine_in(self, n, R, t, which):
        """The input pose as contiguous device tensors (R float32 [n,9] or [n,3,3], t float32 [n,3]): a pose call's output
        as it is, or solution `which` of a homography pose call's [n,2,3,3] / [n,2,3], copied on the device."""
        rm = torch.as_tensor(R).to(self.torch_device, torch.float32)
        tv = torch.as_tensor(t).to(self.torch_device, torch.float32)
        if rm.dim() == 4 or which is not None:
            if which not in (0, 1) or tuple(rm.shape) != (n, 2, 3, 3) or tuple(tv.shape) != (n, 2, 3):
                raise ValueError("which=0 or 1 selects a solution of R [n,2,3,3] and t [n,2,3]")
            rm, tv = rm[:, which], tv[:, which]
        rm, tv = self._guided_h(n, rm, "R"), tv.contiguous()
        if tuple(tv.shape) != (n, 3):
            raise ValueError("t must be [n,3]")
        return rm, tv

    def _refine(self, name, n, pairs, R, t, which, p, stride):
        """fpc_<name> behind its pair source: (R_in, t_in) go in front of the parameters, stats behind the pose outputs."""
        rm, tv = self._refine_in(n, R, t, which)
        stats = torch.empty((n, 4), dtype=torch.float32, device=self.torch_device)
        return self._solve(name, n, pairs, p, self._pose_out(n, stride, True), rm, tv, tail=(stats,))

    def refine_pose_async(self, src, dst, npairs, R, t, K_query=None, K_train=None, which=None, **params):
        """fpc_refine_pose: pose_fundamental_async's pairs and the R, t it returned (device tensors as they are, or host
        arrays; with which=0 / 1 that solution of pose_homography_async's [n,2,3,3] / [n,2,3]) -> device tensors (R float32
        [n,3,3] and t float32 [n,3], refined by a two-view bundle adjustment; nfront int32 [n]; xyz float32 [n,stride,3], the
        refined points; front bool [n,stride]; stats float32 [n,4]: rms reprojection error before and after, attempts made,
        attempts accepted).  Parameters: reproj_threshold, min_parallax_deg, iterations, lambda0, min_front.  A failed frame
        is all zeros.  Does not synchronise."""
        p = self._refine_params(K_query, K_train, params)
        n, pairs = self._explicit_pairs(src, dst, npairs)
        return self._refine("fpc_refine_pose", n, pairs, R, t, which, p, pairs[3])

    def refine_pose(self, src, dst, npairs, R, t, K_query=None, K_train=None, which=None, **params):
        """refine_pose_async, then host arrays (R [n,3,3], t [n,3], nfront [n], xyz [n,stride,3], front bool [n,stride],
        stats [n,4])."""
        return self._host(self.refine_pose_async(src, dst, npairs, R, t, K_query, K_train, which, **params))

    def refine_pose_frames_async(self, n, match, R, t, key_xy=None, pairing="key", K_query=None, K_train=None, which=None,
                                 **params):
        """fpc_refine_pose_frames: pose_frames_async's arguments and pairs with its output R, t -> refine_pose_async's
        tensors with xyz [n,cap,3] and front bool [n,cap] by query row.  Does not synchronise."""
        p, pairs = self._frames_pairs(n, pairing, key_xy, match, self._refine_params, K_query, K_train, params)
        return self._refine("fpc_refine_pose_frames", n, pairs, R, t, which, p, self.capacity)

    def refine_pose_frames(self, n, match, R, t, key_xy=None, pairing="key", K_query=None, K_train=None, which=None, **params):
        """refine_pose_frames_async, then host arrays."""
        return self._host(self.refine_pose_frames_async(n, match, R, t, key_xy, pairing, K_query, K_train, which, **params))

    def refine_pose_bank_async(self, n, slot, match, R, t, K_query=None, K_train=None, which=None, **params):
        """fpc_refine_pose_bank: refine_pose_frames_async with frame f's key coordinates taken from bank slot slot[f], as
        pose_bank_async, whose R, t go in as they are; a frame with slot -1 fails (zeros).  xyz[f] and front[f] go into
        bank_store_landmarks as they are.  Does not synchronise."""
        p, pairs = self._bank_pairs(n, slot, match, self._refine_params, K_query, K_train, params)
        return self._refine("fpc_refine_pose_bank", n, pairs, R, t, which, p, self.capacity)

    def refine_pose_bank(self, n, slot, match, R, t, K_query=None, K_train=None, which=None, **params):
        """refine_pose_bank_async, then host arrays."""
        return self._host(self.refine_pose_bank_async(n, slot, match, R, t, K_query, K_train, which, **params))

    # -- local bundle adjustment of a key frame's landmarks over up to 16 frames (fpc_window_reserve / fpc_refine_window*) -------
    def window_reserve(self):
        """fpc_window_reserve: the window calls' observation table, partial sums and pose state; the only call of the family
        that allocates.  Freed with the engine.  Returns the bytes it allocated."""
        nbytes = ctypes.c_size_t(0)
        _lib.check(self._l.fpc_window_reserve(self._ctx, ctypes.byref(nbytes)), "fpc_window_reserve")
        return int(nbytes.value)

    def _window_params(self, K_query, K_train, params):
        return self._two_camera_params(_lib.FpcWindowParams, "fpc_default_window_params",
                                       ("reproj_threshold", "iterations", "lambda0", "min_obs"), "window", K_query, K_train,
                                       params)

    def _window(self, name, n, source, R, t, p, stride, alias=False):
        """fpc_<name>(ctx, n, *source, R_in, t_in, params, R, t, nobs, xyz, kind, obs, stats) -> (R float32 [n,3,3], t float32
        [n,3], nobs int32 [n], xyz float32 [cap,3], kind uint8 [cap], obs bool [n,stride], stats float32 [4]) on the device.
        alias: R and t are written over the input tensors."""
        rm, tv = self._refine_in(n, R, t, None)
        dev = self.torch_device
        ro = rm.view(n, 3, 3) if alias else torch.empty((n, 3, 3), dtype=torch.float32, device=dev)
        to = tv if alias else torch.empty((n, 3), dtype=torch.float32, device=dev)
        nobs = self._int32(n)
        xyz = torch.empty((self.capacity, 3), dtype=torch.float32, device=dev)
        kind = torch.empty((self.capacity,), dtype=torch.uint8, device=dev)
        obs = torch.empty((n, stride), dtype=torch.uint8, device=dev)
        stats = torch.empty((4,), dtype=torch.float32, device=dev)
        self._call(name, n, *source, rm, tv, ctypes.byref(p), ro, to, nobs, xyz, kind, obs, stats, inputs=(*source, rm, tv))
        return ro, to, nobs, xyz, kind, obs.view(torch.bool), stats

    def refine_window_async(self, xy, idx, nobs, key_xy, key_xyz, R, t, key_valid=None, K_query=None, K_train=None,
                            alias=False, **params):
        """fpc_refine_window: per frame the observed pixels xy (float32 [n,stride,2]) of the key's landmarks idx (int32
        [n,stride]) with nobs int32 [n]; the key's pixels key_xy (float32 [k,2]), its landmarks key_xyz (float32 [k,3], or a
        device pair (xyz, count)) and their flags key_valid (None: every finite row); the poses R, t of fpc_pnp_* -- device
        tensors or host arrays -> device tensors (R [n,3,3], t [n,3], nobs [n], xyz [cap,3], kind uint8 [cap]: 1 refined, 2
        copied unchanged, 0 none; obs bool [n,stride] by pair; stats [4]: rms before, rms after, attempts, accepted).
        Parameters: reproj_threshold, iterations, lambda0, min_obs.  Needs window_reserve.  Does not synchronise."""
        p = self._window_params(K_query, K_train, params)
        xy = torch.as_tensor(xy).to(self.torch_device, torch.float32).contiguous()
        idx = torch.as_tensor(idx).to(self.torch_device, torch.int32).contiguous()
        nobs = torch.as_tensor(nobs).to(self.torch_device, torch.int32).contiguous()
        if xy.dim() != 3 or xy.shape[2] != 2 or idx.shape != xy.shape[:2] or nobs.shape != (xy.shape[0],):
            raise ValueError("xy must be [n,stride,2], idx [n,stride] and nobs [n]")
        n, stride = int(xy.shape[0]), int(xy.shape[1])
        lm, vl, kc = self._key_landmarks(key_xyz, key_valid)
        kx = torch.as_tensor(key_xy).to(self.torch_device, torch.float32).contiguous()
        if kx.dim() != 2 or kx.shape[1] != 2 or kx.shape[0] < lm.shape[0]:
            raise ValueError("key_xy must be [k,2] with a row for each row of key_xyz")
        return self._window("fpc_refine_window", n, (xy, idx, nobs, stride, kx, lm, vl, kc), R, t, p, stride, alias)

    def refine_window(self, xy, idx, nobs, key_xy, key_xyz, R, t, key_valid=None, K_query=None, K_train=None, alias=False,
                      **params):
        """refine_window_async, then host arrays."""
        return self._host(self.refine_window_async(xy, idx, nobs, key_xy, key_xyz, R, t, key_valid, K_query, K_train, alias,
                                                   **params))

    def refine_window_frames_async(self, n, match, R, t, key_xy, key_xyz, key_valid=None, K_query=None, K_train=None,
                                   alias=False, **params):
        """fpc_refine_window_frames: the frames of the last detect with their match table against the key frame whose pixels
        are key_xy and whose landmarks are key_xyz / key_valid (as landmarks_frames_async), under pnp_frames_async's R, t ->
        refine_window_async's outputs, obs bool [n,cap] by query row.  Does not synchronise."""
        p = self._window_params(K_query, K_train, params)
        kx, kc = self._key_xy(key_xy)
        if kx is None:
            raise ValueError("refine_window_frames needs key_xy")
        lm, vl, _ = self._key_landmarks(key_xyz, key_valid)
        if lm.shape[0] < kx.shape[0]:
            raise ValueError("key_xyz needs a row for each row of key_xy")
        match = self._dev_int32("match", match, "[n,%d]" % self.capacity, n, self.capacity)
        return self._window("fpc_refine_window_frames", n, (kx, kc, lm, vl, match), R, t, p, self.capacity, alias)

    def refine_window_frames(self, n, match, R, t, key_xy, key_xyz, key_valid=None, K_query=None, K_train=None, alias=False,
                             **params):
        """refine_window_frames_async, then host arrays."""
        return self._host(self.refine_window_frames_async(n, match, R, t, key_xy, key_xyz, key_valid, K_query, K_train, alias,
                                                          **params))

    def refine_window_bank_async(self, n, key_slot, match, R, t, slot=None, K_query=None, K_train=None, alias=False, **params):
        """fpc_refine_window_bank: refine_window_frames_async with the key's pixels and landmarks taken from bank slot
        key_slot (an int, or a device tensor int32 [1], read on the device); slot (device int32 [n], match_bank_async's best,
        or None): frame f takes part iff slot[f] is the key slot.  `xyz`, `kind` go into bank_store_landmarks(key_slot, xyz,
        kind) as they are.  Does not synchronise."""
        self._bank_info()
        p = self._window_params(K_query, K_train, params)
        if not isinstance(key_slot, torch.Tensor):
            key_slot = torch.tensor([int(key_slot)], dtype=torch.int32, device=self.torch_device)
        key_slot = self._dev_int32("key_slot", key_slot, "[1]", 1)
        if slot is not None:
            slot = self._dev_int32("slot", slot, "[n]", n)
        match = self._dev_int32("match", match, "[n,%d]" % self.capacity, n, self.capacity)
        return self._window("fpc_refine_window_bank", n, (key_slot, slot, match), R, t, p, self.capacity, alias)

    def refine_window_bank(self, n, key_slot, match, R, t, slot=None, K_query=None, K_train=None, alias=False, **params):
        """refine_window_bank_async, then host arrays."""
        return self._host(self.refine_window_bank_async(n, key_slot, match, R, t, slot, K_query, K_train, alias, **params))

    # -- pose graph over the bank's slots (fpc_graph_reserve / _set_nodes / _clear / _get / _add_edges / _optimise / _apply_scale) --
    def graph_reserve(self, nodes, edges):
        """fpc_graph_reserve: Sim(3) nodes (one per bank slot) and room for `edges` edges, with the optimiser's workspace;
        the only graph call that allocates.  Every node starts unset.  Freed with the engine.  Returns the bytes."""
        nbytes = ctypes.c_size_t(0)
        _lib.check(self._l.fpc_graph_reserve(self._ctx, int(nodes), int(edges), ctypes.byref(nbytes)), "fpc_graph_reserve")
        return int(nbytes.value)

    def _graph_view(self):
        v = _lib.FpcGraphView()
        _lib.check(self._l.fpc_graph_get(self._ctx, ctypes.byref(v)), "fpc_graph_get")
        return v

    def _graph_alias(self, ptr, dtype, *shape):
        n = 4
        for s in shape:
            n *= s
        return torch.as_tensor(_DevArray(ptr, n), device=self.torch_device).view(dtype).view(*shape)

    def _dev_f32(self, name, t, *shape):
        """`t` (device tensor or host array) as a contiguous float32 device tensor of `shape`."""
        t = torch.as_tensor(t).to(self.torch_device, torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError("%s must be float32 %s" % (name, list(shape)))
        return t

    def graph_nodes(self):
        """(s float32 [nodes], R float32 [nodes,3,3], t float32 [nodes,3]) aliasing the graph's node state (fpc_graph_get):
        X_i = s_i R_i X_w + t_i; s = 0: the node is unset."""
        v = self._graph_view()
        return (self._graph_alias(v.node_s, torch.float32, v.nodes), self._graph_alias(v.node_R, torch.float32, v.nodes, 3, 3),
                self._graph_alias(v.node_t, torch.float32, v.nodes, 3))

    def graph_edges(self):
        """(from int32 [edges], to int32 [edges], s [edges], R [edges,3,3], t [edges,3], w [edges], count int32 [2])
        aliasing the graph's edge storage: count[0] edges are held, count[1] were dropped for want of room."""
        v = self._graph_view()
        f32, i32, e = torch.float32, torch.int32, v.edges
        return (self._graph_alias(v.edge_from, i32, e), self._graph_alias(v.edge_to, i32, e), self._graph_alias(v.edge_s, f32, e),
                self._graph_alias(v.edge_R, f32, e, 3, 3), self._graph_alias(v.edge_t, f32, e, 3),
                self._graph_alias(v.edge_w, f32, e), self._graph_alias(v.count, i32, 2))

    def graph_clear(self):
        """fpc_graph_clear: every node unset, no edge, both counters zero.  Does not synchronise."""
        self._call("fpc_graph_clear")

    def graph_set_nodes(self, first, R, t, s=None):
        """fpc_graph_set_nodes: nodes first .. first + count - 1 from R [count,3,3], t [count,3] and s [count] (None: 1) --
        device tensors or host arrays.  Does not synchronise."""
        R = torch.as_tensor(R).to(self.torch_device, torch.float32).contiguous()
        if R.dim() != 3 or R.shape[1:] != (3, 3) or R.shape[0] < 1:
            raise ValueError("R must be [count,3,3]")
        count = int(R.shape[0])
        t = self._dev_f32("t", t, count, 3)
        if s is not None:
            s = self._dev_f32("s", s, count)
        self._call("fpc_graph_set_nodes", int(first), count, s, R, t, inputs=(s, R, t))

    def graph_add_edges_async(self, frm, to, R, t, s=None, ninliers=None, min_inliers=0, init_to=False):
        """fpc_graph_add_edges: candidate f measures X_to = s R X_from + t, exactly as pnp_bank_async (s=None) and
        sim3_bank_async write it: frm = the train slot, to = the slot the query frame was or will be stored in (int32 [n],
        device tensors or host arrays), R [n,3,3], t [n,3], s [n] or None, ninliers int32 [n] or None (weight 1).  Failed
        RANSAC outputs (all-zero R), non-finite values, slots out of range and candidates under min_inliers are refused on
        the device; init_to gives an unset `to` node its start from a set `from` node.  Does not synchronise."""
        R = torch.as_tensor(R).to(self.torch_device, torch.float32).contiguous()
        if R.dim() != 3 or R.shape[1:] != (3, 3) or R.shape[0] < 1:
            raise ValueError("R must be [n,3,3]")
        n = int(R.shape[0])
        t = self._dev_f32("t", t, n, 3)
        frm = self._dev_int32("from", torch.as_tensor(frm).to(self.torch_device, torch.int32), "[n]", n)
        to = self._dev_int32("to", torch.as_tensor(to).to(self.torch_device, torch.int32), "[n]", n)
        if s is not None:
            s = self._dev_f32("s", s, n)
        if ninliers is not None:
            ninliers = self._dev_int32("ninliers", torch.as_tensor(ninliers).to(self.torch_device, torch.int32), "[n]", n)
        self._call("fpc_graph_add_edges", n, frm, to, s, R, t, ninliers, int(min_inliers),
                   _lib.GRAPH_INIT_TO if init_to else 0, inputs=(frm, to, s, R, t, ninliers))

    def graph_add_edges(self, frm, to, R, t, s=None, ninliers=None, min_inliers=0, init_to=False):
        """graph_add_edges_async, then (edges held, edges dropped) on the host."""
        self.graph_add_edges_async(frm, to, R, t, s, ninliers, min_inliers, init_to)
        self.sync()
        held, dropped = self.graph_edges()[6].cpu().tolist()
        return held, dropped

    def graph_optimise_async(self, fixed=0, **params):
        """fpc_graph_optimise: Levenberg-Marquardt over the set nodes that have an edge, node `fixed` (an int, or a device
        tensor int32 [1], read on the device) held as the gauge -> stats float32 [4] on the device: cost before, cost after,
        attempts made, attempts accepted; the nodes change in place (graph_nodes).  Parameters: iterations, lambda0,
        cg_iterations, cg_tol, trans_unit.  Does not synchronise."""
        p = self._params(_lib.FpcGraphParams, "fpc_default_graph_params",
                         ("iterations", "lambda0", "cg_iterations", "cg_tol", "trans_unit"), "graph", params)
        if not isinstance(fixed, torch.Tensor):
            fixed = torch.tensor([int(fixed)], dtype=torch.int32, device=self.torch_device)
        fixed = self._dev_int32("fixed", fixed, "[1]", 1)
        stats = torch.empty((4,), dtype=torch.float32, device=self.torch_device)
        self._call("fpc_graph_optimise", fixed, ctypes.byref(p), stats, inputs=(fixed,))
        return stats

    def graph_optimise(self, fixed=0, **params):
        """graph_optimise_async, then the stats on the host."""
        return self._host((self.graph_optimise_async(fixed, **params),))[0]

    def graph_apply_scale(self):
        """fpc_graph_apply_scale: every slot's landmarks, its node and the edges brought to scale 1 (a bank with landmark
        storage and as many slots as the graph has nodes).  Does not synchronise."""
        self._bank_info()
        self._call("fpc_graph_apply_scale")

    # -- absolute pose from landmarks: RANSAC PnP (fpc_pnp_reserve / fpc_bank_*landmarks* / fpc_ransac_pnp / _frames / _bank) ----
    def pnp_reserve(self):
        """fpc_pnp_reserve: the PnP workspace (pair records, counts and best keys of max_batch problems); the only PnP call
        that allocates.  Freed with the engine.  Returns the bytes it allocated."""
        nbytes = ctypes.c_size_t(0)
        _lib.check(self._l.fpc_pnp_reserve(self._ctx, ctypes.byref(nbytes)), "fpc_pnp_reserve")
        return int(nbytes.value)

    def bank_landmarks_reserve(self):
        """fpc_bank_landmarks_reserve: one 3-D point per bank row (float4 [slots,rows], no row valid yet).  Freed with the
        bank.  Returns the bytes it allocated (bank_info()["bytes"] is unchanged)."""
        self._bank_info()
        nbytes = ctypes.c_size_t(0)
        _lib.check(self._l.fpc_bank_landmarks_reserve(self._ctx, ctypes.byref(nbytes)), "fpc_bank_landmarks_reserve")
        return int(nbytes.value)

    def bank_store_landmarks(self, slot, xyz, valid=None):
        """fpc_bank_store_landmarks: the 3-D points of slot `slot`'s rows, in that key frame's camera frame: xyz float32
        [k,3] and valid bool / uint8 [k] with k >= rows (device tensors -- `xyz[f]`, `front[f]` of pose_*_async go in as
        they are -- or host arrays); valid=None: every row.  Call it AFTER the store that filled the slot, which
        invalidates the slot's landmarks.  Does not synchronise."""
        rows = self._bank_info().rows
        xyz = torch.as_tensor(xyz).to(self.torch_device, torch.float32).contiguous()
        if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < rows:
            raise ValueError("xyz must be [k,3] with k >= the bank's rows (%d)" % rows)
        if valid is not None:
            valid = self._dev_uint8(valid)
            if valid.dim() != 1 or valid.shape[0] < rows:
                raise ValueError("valid must be [k] with k >= the bank's rows (%d)" % rows)
        self._call("fpc_bank_store_landmarks", int(slot), xyz, valid, inputs=(xyz, valid))

    def bank_landmarks(self):
        """float32 [slots,rows,4] aliasing the bank's landmark storage (fpc_bank_landmarks_get): (X, Y, Z, w), w = 1 valid
        / 0."""
        v = self._bank_info()
        ptr = ctypes.c_void_p()
        _lib.check(self._l.fpc_bank_landmarks_get(self._ctx, ctypes.byref(ptr)), "fpc_bank_landmarks_get")
        lm = torch.as_tensor(_DevArray(ptr.value, v.slots * v.rows * 16), device=self.torch_device)
        return lm.view(torch.float32).view(v.slots, v.rows, 4)

    def _pnp_params(self, K, params):
        k = self._intrinsics(K, "K")
        p = self._params(_lib.FpcPnpParams, "fpc_default_pnp_params", self._RANSAC_FIELDS, "PnP", params)
        if k is not None:
            p.fx, p.fy, p.cx, p.cy = k
        return p

    def _pnp_out(self, n, stride=None):
        """Empty PnP outputs (R float32 [n,3,3], t float32 [n,3], ninliers int32 [n], mask uint8 [n,stride or cap])."""
        rm, ni, mask = self._ransac_out(n, stride=stride)
        return rm, torch.empty((n, 3), dtype=torch.float32, device=self.torch_device), ni, mask

    def _key_landmarks(self, key_xyz, key_valid):
        """A key frame's 3-D points -> (xyz float32 [k,3], valid uint8 [k] or None, device count) on the device.  key_xyz:
        float32 [k,3] (device or host), or a device pair (xyz, count), used as it is."""
        if isinstance(key_xyz, tuple):
            kx, kc = key_xyz
        else:
            kx = torch.as_tensor(key_xyz).to(self.torch_device, torch.float32).contiguous()
            kc = torch.tensor([kx.shape[0]], dtype=torch.int32, device=self.torch_device)
        if kx.device != self.torch_device or kx.dtype != torch.float32 or kx.dim() != 2 or kx.shape[1] != 3 \
                or kc.device != self.torch_device or kc.dtype != torch.int32:
            raise ValueError("key_xyz must be float32 [k,3], or device tensors (float32 [k,3], int32 [1])")
        kx = kx.contiguous()
        kv = None
        if key_valid is not None:
            kv = self._dev_uint8(key_valid)
            if kv.dim() != 1 or kv.shape[0] < kx.shape[0]:
                raise ValueError("key_valid must be [k]")
        return kx, kv, kc

    def ransac_pnp_async(self, xy, xyz, npairs, K=None, **params):
        """fpc_ransac_pnp: xy float32 [n,stride,2] pixels, xyz float32 [n,stride,3] points and npairs int32 [n] (device
        tensors or host arrays) -> device tensors (R float32 [n,3,3] and t float32 [n,3] with X_cam = R X + t, ninliers
        int32 [n], inlier bool [n,stride]); a failed frame is all zeros.  K: the camera as a 3 x 3 matrix or (fx, fy, cx,
        cy).  Parameters: the other fields of fpc_pnp_params.  Needs pnp_reserve().  Does not synchronise."""
        return self._pose_explicit("fpc_ransac_pnp", xy, xyz, npairs, K, params)

    # the three pair sources of the absolute-pose calls, for either model (`name`: the DLT's call or its P3P twin)
    def _pose_explicit(self, name, xy, xyz, npairs, K, params):
        p = self._pnp_params(K, params)
        n, pairs = self._explicit_pairs(xy, xyz, npairs, 3, "xy must be [n,stride,2], xyz [n,stride,3] and npairs [n]")
        return self._solve(name, n, pairs, p, self._pnp_out(n, pairs[3]))

    def _pose_frames(self, name, n, match, key_xyz, key_valid, K, params):
        p = self._pnp_params(K, params)
        kx, kv, kc = self._key_landmarks(key_xyz, key_valid)
        match = self._dev_int32("match", match, "[n,%d]" % self.capacity, n, self.capacity)
        return self._solve(name, n, (kx, kv, kc, match), p, self._pnp_out(n))

    def _pose_bank(self, name, n, slot, match, K, params):
        p, pairs = self._bank_pairs(n, slot, match, self._pnp_params, K, params)
        return self._solve(name, n, pairs, p, self._pnp_out(n))

    def ransac_pnp(self, xy, xyz, npairs, K=None, **params):
        """ransac_pnp_async, then host arrays (R [n,3,3], t [n,3], ninliers [n], inlier bool [n,stride])."""
        return self._host(self.ransac_pnp_async(xy, xyz, npairs, K, **params))

    def pnp_frames_async(self, n, match, key_xyz, key_valid=None, K=None, **params):
        """fpc_pnp_frames: the pairs (xy[f][i], key_xyz[match[f][i]]) of every frame of the last detect, `match` being
        match_frames_async's table against the key frame whose rows' 3-D points are key_xyz (float32 [k,3], or a device
        pair (xyz, count)) and key_valid (bool / uint8 [k], None: every row) -> device tensors (R [n,3,3], t [n,3],
        ninliers [n], inlier bool [n,cap] by query row).  Does not synchronise."""
        return self._pose_frames("fpc_pnp_frames", n, match, key_xyz, key_valid, K, params)

    def pnp_frames(self, n, match, key_xyz, key_valid=None, K=None, **params):
        """pnp_frames_async, then host arrays (R [n,3,3], t [n,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.pnp_frames_async(n, match, key_xyz, key_valid, K, **params))

    def pnp_bank_async(self, n, slot, match, K=None, **params):
        """fpc_pnp_bank: pnp_frames_async with frame f's landmarks taken from bank slot slot[f] (int32 [n], device; normally
        match_bank_async's `best`) and `match` that call's table; a frame with slot -1, or a bank without landmarks, fails
        (zeros).  Does not synchronise."""
        return self._pose_bank("fpc_pnp_bank", n, slot, match, K, params)

    def pnp_bank(self, n, slot, match, K=None, **params):
        """pnp_bank_async, then host arrays (R [n,3,3], t [n,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.pnp_bank_async(n, slot, match, K, **params))

    # -- absolute pose from a minimal sample: P3P + 1 (fpc_ransac_p3p / _frames / _bank) --------------------------------------
    # The twins of the six calls above: the same arguments, parameters (min_inliers may go down to 4) and returns, with a
    # sample of four pairs that coplanar landmarks -- those of a pose_homography_* call -- do not defeat.
    def ransac_p3p_async(self, xy, xyz, npairs, K=None, **params):
        """fpc_ransac_p3p: ransac_pnp_async with the minimal-sample model.  Needs pnp_reserve().  Does not synchronise."""
        return self._pose_explicit("fpc_ransac_p3p", xy, xyz, npairs, K, params)

    def ransac_p3p(self, xy, xyz, npairs, K=None, **params):
        """ransac_p3p_async, then host arrays (R [n,3,3], t [n,3], ninliers [n], inlier bool [n,stride])."""
        return self._host(self.ransac_p3p_async(xy, xyz, npairs, K, **params))

    def p3p_frames_async(self, n, match, key_xyz, key_valid=None, K=None, **params):
        """fpc_p3p_frames: pnp_frames_async with the minimal-sample model.  Does not synchronise."""
        return self._pose_frames("fpc_p3p_frames", n, match, key_xyz, key_valid, K, params)

    def p3p_frames(self, n, match, key_xyz, key_valid=None, K=None, **params):
        """p3p_frames_async, then host arrays (R [n,3,3], t [n,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.p3p_frames_async(n, match, key_xyz, key_valid, K, **params))

    def p3p_bank_async(self, n, slot, match, K=None, **params):
        """fpc_p3p_bank: pnp_bank_async with the minimal-sample model.  Does not synchronise."""
        return self._pose_bank("fpc_p3p_bank", n, slot, match, K, params)

    def p3p_bank(self, n, slot, match, K=None, **params):
        """p3p_bank_async, then host arrays (R [n,3,3], t [n,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.p3p_bank_async(n, slot, match, K, **params))

    # -- map growth: landmarks for a new key frame from its PnP pose (fpc_landmarks_pairs / _frames / _bank) -----------------
    def _landmark_params(self, K_query, K_train, params):
        return self._two_camera_params(_lib.FpcLandmarkParams, "fpc_default_landmark_params",
                                       ("reproj_threshold", "min_parallax_deg"), "landmark", K_query, K_train, params)

    def _landmarks(self, name, n, pairs, R, t, p, stride):
        """fpc_<name>(ctx, n, *pairs, R, t, params, xyz, kind, counts) -> (xyz float32 [n,stride,3], kind uint8 [n,stride],
        counts int32 [n,2]) on the device."""
        rm = self._guided_h(n, R, "R")
        tv = torch.as_tensor(t).to(self.torch_device, torch.float32).contiguous()
        if tuple(tv.shape) != (n, 3):
            raise ValueError("t must be [n,3]")
        xyz = torch.empty((n, stride, 3), dtype=torch.float32, device=self.torch_device)
        kind = torch.empty((n, stride), dtype=torch.uint8, device=self.torch_device)
        counts = self._int32(n, 2)
        self._call(name, n, *pairs, rm, tv, ctypes.byref(p), xyz, kind, counts, inputs=(*pairs, rm, tv))
        return xyz, kind, counts

    def landmarks_pairs_async(self, q_xy, t_xy, npairs, R, t, t_xyz=None, t_valid=None, K_query=None, K_train=None,
                              **params):
        """fpc_landmarks_pairs: per pair the query pixel q_xy and the train pixel t_xy (float32 [n,stride,2]), the train
        row's 3-D point t_xyz (float32 [n,stride,3]; None: no row has one) and its flag t_valid (bool / uint8 [n,stride];
        None: every finite row), npairs int32 [n] -- device tensors or host arrays -- under the poses R (float32 [n,3,3] or
        [n,9]) and t (float32 [n,3]) with X_query = R X_train + t, the PnP calls' output -> device tensors (xyz float32
        [n,stride,3] in the query camera's frame, kind uint8 [n,stride]: 1 carried over, 2 triangulated, 0 neither; counts
        int32 [n,2] of kinds 1 and 2).  K_query / K_train: 3 x 3 camera matrices or (fx, fy, cx, cy).  Parameters:
        reproj_threshold, min_parallax_deg.  A frame with a failed pose is all zeros.  Does not synchronise."""
        p = self._landmark_params(K_query, K_train, params)
        n, (a, b, npairs, stride) = self._explicit_pairs(q_xy, t_xy, npairs, 2,
                                                         "q_xy and t_xy must be [n,stride,2] and npairs [n]")
        lm = vl = None
        if t_xyz is not None:
            lm = torch.as_tensor(t_xyz).to(self.torch_device, torch.float32).contiguous()
            if tuple(lm.shape) != (n, stride, 3):
                raise ValueError("t_xyz must be [n,stride,3]")
        if t_valid is not None:
            vl = self._dev_uint8(t_valid)
            if tuple(vl.shape) != (n, stride):
                raise ValueError("t_valid must be [n,stride]")
        return self._landmarks("fpc_landmarks_pairs", n, (a, b, lm, vl, npairs, stride), R, t, p, stride)

    def landmarks_pairs(self, q_xy, t_xy, npairs, R, t, t_xyz=None, t_valid=None, K_query=None, K_train=None, **params):
        """landmarks_pairs_async, then host arrays (xyz [n,stride,3], kind uint8 [n,stride], counts [n,2])."""
        return self._host(self.landmarks_pairs_async(q_xy, t_xy, npairs, R, t, t_xyz, t_valid, K_query, K_train, **params))

    def landmarks_frames_async(self, n, match, R, t, key_xy, key_xyz=None, key_valid=None, K_query=None, K_train=None,
                               **params):
        """fpc_landmarks_frames: the rows (xy[f][i], key row match[f][i]) of every frame of the last detect, `match` being
        match_frames_async's table against the key frame whose pixels are key_xy (keep_frame_points, or an (xy, count)
        device pair) and whose rows' 3-D points are key_xyz / key_valid as in pnp_frames_async (None: the key has none, every
        row is triangulated); R, t: pnp_frames_async's output -> device tensors (xyz [n,cap,3], kind uint8 [n,cap] by query
        row, counts [n,2]); `xyz[f]`, `kind[f]` go into bank_store_landmarks as they are.  Does not synchronise."""
        p = self._landmark_params(K_query, K_train, params)
        kx, kc = self._key_xy(key_xy)
        if kx is None:
            raise ValueError("landmarks_frames needs key_xy")
        lm = vl = None
        if key_xyz is not None:
            lm, vl, _ = self._key_landmarks(key_xyz, key_valid)
            if lm.shape[0] < kx.shape[0]:
                raise ValueError("key_xyz needs a row for each row of key_xy")
        match = self._dev_int32("match", match, "[n,%d]" % self.capacity, n, self.capacity)
        return self._landmarks("fpc_landmarks_frames", n, (kx, kc, lm, vl, match), R, t, p, self.capacity)

    def landmarks_frames(self, n, match, R, t, key_xy, key_xyz=None, key_valid=None, K_query=None, K_train=None, **params):
        """landmarks_frames_async, then host arrays (xyz [n,cap,3], kind uint8 [n,cap], counts [n,2])."""
        return self._host(self.landmarks_frames_async(n, match, R, t, key_xy, key_xyz, key_valid, K_query, K_train, **params))

    def landmarks_bank_async(self, n, slot, match, R, t, K_query=None, K_train=None, **params):
        """fpc_landmarks_bank: landmarks_frames_async with frame f's key pixels and landmarks taken from bank slot slot[f]
        (as pnp_bank_async, whose R, t go in as they are) on a bank of either format; a frame with slot -1 is all zeros; a
        bank without landmarks triangulates every row.  bank_store(f, s) and bank_store_landmarks(s, xyz[f], kind[f]) behind
        it make frame f the next key frame, at the map's scale.  Does not synchronise."""
        p, pairs = self._bank_pairs(n, slot, match, self._landmark_params, K_query, K_train, params)
        return self._landmarks("fpc_landmarks_bank", n, pairs, R, t, p, self.capacity)

    def landmarks_bank(self, n, slot, match, R, t, K_query=None, K_train=None, **params):
        """landmarks_bank_async, then host arrays (xyz [n,cap,3], kind uint8 [n,cap], counts [n,2])."""
        return self._host(self.landmarks_bank_async(n, slot, match, R, t, K_query, K_train, **params))

    # -- Sim(3) alignment between two frames' landmarks (fpc_ransac_sim3 / fpc_sim3_frames / fpc_sim3_bank) ---------------------
    def _sim3_params(self, K_query, K_train, params):
        return self._two_camera_params(_lib.FpcSim3Params, "fpc_default_sim3_params", self._RANSAC_FIELDS + ("fix_scale",),
                                       "Sim(3)", K_query, K_train, params)

    def _sim3_out(self, n, stride=None):
        """Empty Sim(3) outputs (s float32 [n], R float32 [n,3,3], t float32 [n,3], ninliers int32 [n], mask uint8
        [n,stride or cap])."""
        rm, tv, ni, mask = self._pnp_out(n, stride)
        return torch.empty((n,), dtype=torch.float32, device=self.torch_device), rm, tv, ni, mask

    def _query_landmarks(self, n, q_xyz, q_valid):
        """The frames' own landmarks -> (xyz float32 [n,cap,3], valid uint8 [n,cap] or None) on the device: xyz and kind of
        landmarks_*_async, used as they are."""
        cap = self.capacity
        qx = torch.as_tensor(q_xyz).to(self.torch_device, torch.float32).contiguous()
        if tuple(qx.shape) != (n, cap, 3):
            raise ValueError("q_xyz must be [n,%d,3]" % cap)
        qv = None
        if q_valid is not None:
            qv = self._dev_uint8(q_valid)
            if tuple(qv.shape) != (n, cap):
                raise ValueError("q_valid must be [n,%d]" % cap)
        return qx, qv

    def ransac_sim3_async(self, q_xyz, t_xyz, npairs, K_query=None, K_train=None, **params):
        """fpc_ransac_sim3: q_xyz and t_xyz float32 [n,stride,3], the pairs' points in the query and the train camera's
        frame, and npairs int32 [n] (device tensors or host arrays) -> device tensors (s float32 [n], R float32 [n,3,3] and
        t float32 [n,3] with X_query = s R X_train + t, ninliers int32 [n], inlier bool [n,stride]); a failed frame is all
        zeros.  K_query / K_train: 3 x 3 camera matrices or (fx, fy, cx, cy).  Parameters: the other fields of
        fpc_sim3_params.  Needs pnp_reserve().  Does not synchronise."""
        p = self._sim3_params(K_query, K_train, params)
        n, pairs = self._explicit_pairs(q_xyz, t_xyz, npairs, 3, "q_xyz and t_xyz must be [n,stride,3] and npairs [n]", 3)
        return self._solve("fpc_ransac_sim3", n, pairs, p, self._sim3_out(n, pairs[3]))

    def ransac_sim3(self, q_xyz, t_xyz, npairs, K_query=None, K_train=None, **params):
        """ransac_sim3_async, then host arrays (s [n], R [n,3,3], t [n,3], ninliers [n], inlier bool [n,stride])."""
        return self._host(self.ransac_sim3_async(q_xyz, t_xyz, npairs, K_query, K_train, **params))

    def sim3_frames_async(self, n, match, q_xyz, q_valid, key_xyz, key_valid=None, K_query=None, K_train=None, **params):
        """fpc_sim3_frames: the pairs (q_xyz[f][i], key_xyz[match[f][i]]) of every frame of the last detect: q_xyz float32
        [n,cap,3] and q_valid (bool / uint8 [n,cap], None: every row) the frames' own landmarks -- xyz and kind of
        landmarks_*_async as they are --, `match` match_frames_async's table against the key frame whose landmarks are
        key_xyz / key_valid as in pnp_frames_async -> device tensors (s [n], R [n,3,3], t [n,3], ninliers [n], inlier bool
        [n,cap] by query row).  Does not synchronise."""
        p = self._sim3_params(K_query, K_train, params)
        qx, qv = self._query_landmarks(n, q_xyz, q_valid)
        kx, kv, kc = self._key_landmarks(key_xyz, key_valid)
        match = self._dev_int32("match", match, "[n,%d]" % self.capacity, n, self.capacity)
        return self._solve("fpc_sim3_frames", n, (qx, qv, kx, kv, kc, match), p, self._sim3_out(n))

    def sim3_frames(self, n, match, q_xyz, q_valid, key_xyz, key_valid=None, K_query=None, K_train=None, **params):
        """sim3_frames_async, then host arrays (s [n], R [n,3,3], t [n,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.sim3_frames_async(n, match, q_xyz, q_valid, key_xyz, key_valid, K_query, K_train, **params))

    def sim3_bank_async(self, n, slot, match, q_xyz, q_valid=None, K_query=None, K_train=None, **params):
        """fpc_sim3_bank: sim3_frames_async with frame f's train landmarks taken from bank slot slot[f] (int32 [n], device;
        a loop candidate of match_bank_topk_async, say) and `match` the table against that slot, on a bank of either format;
        a frame with slot -1, or a bank without landmarks, fails (zeros).  s is the ratio of the frame's scale to the
        slot's: the drift between the two.  Does not synchronise."""
        p, pairs = self._bank_pairs(n, slot, match, self._sim3_params, K_query, K_train, params)
        qx, qv = self._query_landmarks(n, q_xyz, q_valid)
        return self._solve("fpc_sim3_bank", n, (qx, qv, *pairs), p, self._sim3_out(n))

    def sim3_bank(self, n, slot, match, q_xyz, q_valid=None, K_query=None, K_train=None, **params):
        """sim3_bank_async, then host arrays (s [n], R [n,3,3], t [n,3], ninliers [n], inlier bool [n,cap])."""
        return self._host(self.sim3_bank_async(n, slot, match, q_xyz, q_valid, K_query, K_train, **params))

    # -- verified relocalisation: the k best slots per frame, each checked by RANSAC (fpc_*_bank_topk) ------------------
    def bank_topk_reserve(self, kmax):
        """fpc_bank_topk_reserve: workspace for up to `kmax` candidates per frame (1 <= kmax <= min(16, slots)); the only
        top-K call that allocates.  Freed with the bank.  Returns the bytes it allocated (bank_info()["bytes"] is
        unchanged)."""
        self._bank_info()
        nbytes = ctypes.c_size_t(0)
        _lib.check(self._l.fpc_bank_topk_reserve(self._ctx, int(kmax), ctypes.byref(nbytes)), "fpc_bank_topk_reserve")
        self._topk_kmax = int(kmax)
        return int(nbytes.value)

    def match_bank_topk_async(self, n, k, cross_check=True, max_dist=0.0, ratio=0.0, min_score=0, table=True):
        """fpc_match_bank_topk: match_bank_async's scores and, per frame, the k best slots in descending (score, lower slot
        first) order -> device tensors (score int32 [n,slots], cand_slot int32 [n,k] (-1: fewer than k slots reached
        max(min_score, 1)), cand_score int32 [n,k], match int32 [n,k,cap], dist float32 [n,k,cap]) -- the last two are the
        table of frame f against slot cand_slot[f,j] (None with table=False).  Does not synchronise."""
        v = self._bank_info()
        k = int(k)
        score, cs, csc = self._int32(n, v.slots), self._int32(n, k), self._int32(n, k)
        m, d = self._table(n, k) if table else (None, None)
        self._call("fpc_match_bank_topk", n, k, int(bool(cross_check)), float(max_dist), float(ratio), int(min_score), score,
                   cs, csc, m, d)
        return score, cs, csc, m, d

    def match_bank_topk(self, n, k, cross_check=True, max_dist=0.0, ratio=0.0, min_score=0):
        """match_bank_topk_async, then host arrays (score [n,slots], cand_slot [n,k], cand_score [n,k], match [n,k,cap],
        dist [n,k,cap])."""
        return self._host(self.match_bank_topk_async(n, k, cross_check, max_dist, ratio, min_score))

    def homography_bank_topk_async(self, n, cand_slot, match, **params):
        """fpc_homography_bank_topk: homography_bank_async for every candidate -- cand_slot int32 [n,k] and match int32
        [n,k,cap] are match_bank_topk_async's -> device tensors (H [n,k,3,3], ninliers [n,k], inlier bool [n,k,cap], pick
        int32 [n]: the candidate with the most inliers, ties to the lower j, -1: none; best int32 [n]: its slot, or -1).
        Does not synchronise."""
        self._bank_info()
        p = self._ransac_params(params)
        cand_slot = self._dev_int32("cand_slot", cand_slot, "[n,k]", n, None)
        k = int(cand_slot.shape[1])
        match = self._dev_int32("match", match, "[n,k,%d]" % self.capacity, n, k, self.capacity)
        hm, ni, mask = self._ransac_out(n, k)
        pick, best = self._int32(n), self._int32(n)
        self._call("fpc_homography_bank_topk", n, k, cand_slot, match, ctypes.byref(p), hm, ni, mask, pick, best,
                   inputs=(cand_slot, match))
        return hm, ni, mask.view(torch.bool), pick, best

    def homography_bank_topk(self, n, cand_slot, match, **params):
        """homography_bank_topk_async, then host arrays (H [n,k,3,3], ninliers [n,k], inlier bool [n,k,cap], pick [n],
        best [n])."""
        return self._host(self.homography_bank_topk_async(n, cand_slot, match, **params))

    def relocalise(self, n, k, cross_check=True, max_dist=0.7, ratio=0.0, min_score=0, **params):
        """match_bank_topk_async then homography_bank_topk_async, one synchronisation: which stored frame does each frame
        see, verified geometrically -> host arrays (best [n]: the candidate slot with the most inliers, -1: none verified;
        H [n,k,3,3] and ninliers [n,k] of every candidate; cand_slot [n,k]; cand_score [n,k]).  Needs bank_topk_reserve(kmax
        >= k); RANSAC parameters as in homography_bank_async."""
        _, cs, csc, m, _ = self.match_bank_topk_async(n, k, cross_check, max_dist, ratio, min_score)
        hm, ni, _, _, best = self.homography_bank_topk_async(n, cs, m, **params)
        return self._host((best, hm, ni, cs, csc))

    # -- verified relocalisation by pose: every candidate under PnP, P3P, F or E (fpc_pnp_topk_reserve / fpc_*_bank_topk) ----
    def pnp_topk_reserve(self):
        """fpc_pnp_topk_reserve: the absolute-pose workspace of max_batch x kmax (frame, candidate) problems, kmax being
        bank_topk_reserve's; the only call of pnp_bank_topk / p3p_bank_topk that allocates (no pnp_reserve is needed).
        Freed with the bank.  Returns the bytes it allocated (bank_info()["bytes"] is unchanged)."""
        self._bank_info()
        nbytes = ctypes.c_size_t(0)
        _lib.check(self._l.fpc_pnp_topk_reserve(self._ctx, ctypes.byref(nbytes)), "fpc_pnp_topk_reserve")
        return int(nbytes.value)

    def _topk_pairs(self, n, cand_slot, match, fill, *args):
        """The top-K pair source -> (fill(*args), k, cand_slot int32 [n,k], match int32 [n,k,cap]), behind the check that a
        bank exists."""
        self._bank_info()
        p = fill(*args)
        cand_slot = self._dev_int32("cand_slot", cand_slot, "[n,k]", n, None)
        k = int(cand_slot.shape[1])
        return p, k, cand_slot, self._dev_int32("match", match, "[n,k,%d]" % self.capacity, n, k, self.capacity)

    def _pose_bank_topk(self, name, n, cand_slot, match, K, params):
        p, k, cand_slot, match = self._topk_pairs(n, cand_slot, match, self._pnp_params, K, params)
        rm, ni, mask = self._ransac_out(n, k)
        tv = torch.empty((n, k, 3), dtype=torch.float32, device=self.torch_device)
        pick, best = self._int32(n), self._int32(n)
        best_r = torch.empty((n, 3, 3), dtype=torch.float32, device=self.torch_device)
        best_t = torch.empty((n, 3), dtype=torch.float32, device=self.torch_device)
        self._call(name, n, k, cand_slot, match, ctypes.byref(p), rm, tv, ni, mask, pick, best, best_r, best_t,
                   inputs=(cand_slot, match))
        return rm, tv, ni, mask.view(torch.bool), pick, best, best_r, best_t

    def pnp_bank_topk_async(self, n, cand_slot, match, K=None, **params):
        """fpc_pnp_bank_topk: pnp_bank_async for every candidate -- cand_slot int32 [n,k] and match int32 [n,k,cap] are
        match_bank_topk_async's -> device tensors (R [n,k,3,3], t [n,k,3], ninliers [n,k], inlier bool [n,k,cap], pick
        int32 [n]: the candidate with the most inliers, ties to the lower j, -1: none; best int32 [n]: its slot, or -1;
        best_R [n,3,3] and best_t [n,3]: its pose, zeros where pick is -1).  Column j is bit-identical to
        pnp_bank_async(n, cand_slot[:, j], match[:, j]).  K and the parameters as in pnp_bank_async.  Needs
        pnp_topk_reserve().  Does not synchronise."""
        return self._pose_bank_topk("fpc_pnp_bank_topk", n, cand_slot, match, K, params)

    def pnp_bank_topk(self, n, cand_slot, match, K=None, **params):
        """pnp_bank_topk_async, then host arrays (R [n,k,3,3], t [n,k,3], ninliers [n,k], inlier bool [n,k,cap], pick [n],
        best [n], best_R [n,3,3], best_t [n,3])."""
        return self._host(self.pnp_bank_topk_async(n, cand_slot, match, K, **params))

    def p3p_bank_topk_async(self, n, cand_slot, match, K=None, **params):
        """fpc_p3p_bank_topk: pnp_bank_topk_async with the minimal-sample model (p3p_bank_async for every candidate).  Does
        not synchronise."""
        return self._pose_bank_topk("fpc_p3p_bank_topk", n, cand_slot, match, K, params)

    def p3p_bank_topk(self, n, cand_slot, match, K=None, **params):
        """p3p_bank_topk_async, then host arrays (R [n,k,3,3], t [n,k,3], ninliers [n,k], inlier bool [n,k,cap], pick [n],
        best [n], best_R [n,3,3], best_t [n,3])."""
        return self._host(self.p3p_bank_topk_async(n, cand_slot, match, K, **params))

    def fundamental_bank_topk_async(self, n, cand_slot, match, **params):
        """fpc_fundamental_bank_topk: fundamental_bank_async for every candidate, arguments as homography_bank_topk_async
        -> device tensors (F [n,k,3,3], ninliers [n,k], inlier bool [n,k,cap], pick int32 [n], best int32 [n], best_F
        [n,3,3]: the picked candidate's F, zeros where pick is -1 -- what match_bank_guided_epipolar_async(best, best_F)
        and pose_bank_async take).  A wrong candidate still collects chance inliers under an epipolar model: min_inliers
        is the caller's floor.  Needs bank_topk_reserve() only.  Does not synchronise."""
        p, k, cand_slot, match = self._topk_pairs(n, cand_slot, match, self._ransac_params, params)
        fm, ni, mask = self._ransac_out(n, k)
        pick, best = self._int32(n), self._int32(n)
        best_f = torch.empty((n, 3, 3), dtype=torch.float32, device=self.torch_device)
        self._call("fpc_fundamental_bank_topk", n, k, cand_slot, match, ctypes.byref(p), fm, ni, mask, pick, best, best_f,
                   inputs=(cand_slot, match))
        return fm, ni, mask.view(torch.bool), pick, best, best_f

    def fundamental_bank_topk(self, n, cand_slot, match, **params):
        """fundamental_bank_topk_async, then host arrays (F [n,k,3,3], ninliers [n,k], inlier bool [n,k,cap], pick [n],
        best [n], best_F [n,3,3])."""
        return self._host(self.fundamental_bank_topk_async(n, cand_slot, match, **params))

    def essential_bank_topk_async(self, n, cand_slot, match, K_query=None, K_train=None, **params):
        """fpc_essential_bank_topk: essential_bank_async for every candidate -> device tensors (F [n,k,3,3], E [n,k,3,3],
        ninliers [n,k], inlier bool [n,k,cap], pick int32 [n], best int32 [n], best_F [n,3,3]), as
        fundamental_bank_topk_async; the cameras and parameters as in essential_bank_async.  Does not synchronise."""
        p, k, cand_slot, match = self._topk_pairs(n, cand_slot, match, self._essential_params, K_query, K_train, params)
        fm, ni, mask = self._ransac_out(n, k)
        em = torch.empty_like(fm)
        pick, best = self._int32(n), self._int32(n)
        best_f = torch.empty((n, 3, 3), dtype=torch.float32, device=self.torch_device)
        self._call("fpc_essential_bank_topk", n, k, cand_slot, match, ctypes.byref(p), fm, em, ni, mask, pick, best, best_f,
                   inputs=(cand_slot, match))
        return fm, em, ni, mask.view(torch.bool), pick, best, best_f

    def essential_bank_topk(self, n, cand_slot, match, K_query=None, K_train=None, **params):
        """essential_bank_topk_async, then host arrays (F [n,k,3,3], E [n,k,3,3], ninliers [n,k], inlier bool [n,k,cap],
        pick [n], best [n], best_F [n,3,3])."""
        return self._host(self.essential_bank_topk_async(n, cand_slot, match, K_query, K_train, **params))

    def relocalise_pose(self, n, k, K=None, model="p3p", radius=8.0, cross_check=True, max_dist=0.7, ratio=0.0, min_score=0,
                        **params):
        """The pose of every frame against the map, over the k best slots: match_bank_topk_async, then p3p_bank_topk_async
        (model "p3p") or pnp_bank_topk_async ("pnp") on every candidate, then match_bank_guided_pose_async(best, best_R,
        best_t, radius) -- the picked slot once more, by projection -- and pnp_bank_async(best) on that table; one
        synchronisation, no host call in between -> host arrays (best [n]: the picked slot, -1: none verified; R [n,3,3], t
        [n,3], ninliers [n], inlier bool [n,cap]: the final pose, zeros where best is -1; then every candidate's: cand_R
        [n,k,3,3], cand_t [n,k,3], cand_ninliers [n,k], pick [n], cand_slot [n,k], cand_score [n,k]).  K and the
        parameters go to both pose calls (min_inliers >= 6 for the second).  Needs an "f32" bank with landmarks,
        bank_topk_reserve(kmax >= k), pnp_topk_reserve() and pnp_reserve()."""
        if model not in ("pnp", "p3p"):
            raise ValueError("model must be 'pnp' or 'p3p', got %r" % (model,))
        if self.bank_info()["format"] != "f32":           # before anything is launched: the chain's third call would refuse it
            raise ValueError("relocalise_pose needs an 'f32' bank: match_bank_guided_pose has no 'bf16' gate")
        pose_topk = self.p3p_bank_topk_async if model == "p3p" else self.pnp_bank_topk_async
        _, cs, csc, m, _ = self.match_bank_topk_async(n, k, cross_check, max_dist, ratio, min_score)
        rk, tk, nk, _, pick, best, best_r, best_t = pose_topk(n, cs, m, K, **params)
        m2, _ = self.match_bank_guided_pose_async(n, best, best_r, best_t, radius, K, cross_check, max_dist, ratio)
        rm, tv, ni, mask = self.pnp_bank_async(n, best, m2, K, **params)
        return self._host((best, rm, tv, ni, mask, rk, tk, nk, pick, cs, csc))

    # -- guided matching: the match once more under the estimated homographies (fpc_match_*_guided), and its cell-ordered
    # -- form (fpc_cell_order / fpc_match_*_guided_cells): the same tables, fewer tiles ------------------------------------
    def _guided_h(self, n, hm, what="H"):
        """H (or F) -> a contiguous device tensor float32 [n,9] (homography_*_async's / fundamental_*_async's [n,3,3] output
        as it is, or a host array)."""
        hm = torch.as_tensor(hm).to(self.torch_device, torch.float32).contiguous()
        if hm.numel() != n * 9 or hm.shape[0] != n:
            raise ValueError("%s must be [n,3,3] or [n,9]" % what)
        return hm

    def _guided(self, name, variant, stats, n, train, H, radius, cross_check, max_dist, ratio):
        """fpc_<name><variant>(ctx, n, *train, H, radius, ...): what every guided call does behind its train set's checks.
        variant: "" (the plain call), "_cells" (takes stats_dev as well), "_epipolar" (H is then F) or "_epipolar_cells"
        (both)."""
        cells = variant.endswith("_cells")
        hm = self._guided_h(n, H, "F" if variant.startswith("_epipolar") else "H")
        m, d = self._table(n)
        st = self._int32(n, 2) if stats else None
        self._call(name + variant, n, *train, hm, float(radius), int(bool(cross_check)), float(max_dist),
                   float(ratio), m, d, *((st,) if cells else ()), inputs=(*train, hm))
        return (m, d, st) if stats else (m, d)

    def _guided_frames(self, variant, stats, n, H, radius, key, key_xy, pairing, *options):
        pair = self._pairing(pairing)
        kd, kc = self._key(key)
        kx, _ = self._key_xy(key_xy)
        if kd is not None and (kx is None or kx.shape[0] < kd.shape[0]):
            raise ValueError("a key needs key_xy with a row for each of its rows")
        return self._guided("fpc_match_frames_guided", variant, stats, n, (pair, kd, kc, kx), H, radius, *options)

    def _guided_bank(self, variant, stats, n, slot, H, radius, *options):
        self._bank_info()
        slot = self._dev_int32("slot", slot, "[n]", n)
        return self._guided("fpc_match_bank_guided", variant, stats, n, (slot,), H, radius, *options)

    def match_frames_guided_async(self, n, H, radius, key=None, key_xy=None, pairing="key", cross_check=True, max_dist=0.0,
                                  ratio=0.0):
        """fpc_match_frames_guided: match_frames_async over the train rows within `radius` pixels of where H[f] (float32
        [n,3,3], query pixel -> train pixel: homography_frames_async's output, device or host) sends the query row;
        `key` / `key_xy` as in match_frames_async / homography_frames_async (the key's count is `key`'s) -> (match int32
        [n,cap], dist float32 [n,cap]) on the device; a frame with H = 0 is all -1.  Does not synchronise."""
        return self._guided_frames("", False, n, H, radius, key, key_xy, pairing, cross_check, max_dist, ratio)

    def match_frames_guided(self, n, H, radius, key=None, key_xy=None, pairing="key", cross_check=True, max_dist=0.0,
                            ratio=0.0):
        """match_frames_guided_async, then per frame (match int32 [K_f], dist float32 [K_f])."""
        return self._per_frame(n, *self.match_frames_guided_async(n, H, radius, key, key_xy, pairing, cross_check,
                                                                  max_dist, ratio))

    def match_bank_guided_async(self, n, slot, H, radius, cross_check=True, max_dist=0.0, ratio=0.0):
        """fpc_match_bank_guided: match_frames_guided_async with frame f's train set taken from bank slot slot[f] (int32
        [n], device; normally match_bank_async's `best`; -1: an all -1 row) and H homography_bank_async's output.  Does
        not synchronise."""
        return self._guided_bank("", False, n, slot, H, radius, cross_check, max_dist, ratio)

    def match_bank_guided(self, n, slot, H, radius, cross_check=True, max_dist=0.0, ratio=0.0):
        """match_bank_guided_async, then per frame (match int32 [K_f], dist float32 [K_f])."""
        return self._per_frame(n, *self.match_bank_guided_async(n, slot, H, radius, cross_check, max_dist, ratio))

    def cell_order_async(self, xy, counts):
        """fpc_cell_order: xy int32 [sets,stride,2], counts int32 [sets] (device tensors or host arrays) -> perm int32
        [sets,stride] on the device: every set's rows in the stable order by 32-px cell (include/fpc.h); entries past a
        set's count are unspecified.  Does not synchronise."""
        xy = torch.as_tensor(xy).to(self.torch_device, torch.int32).contiguous()
        counts = torch.as_tensor(counts).to(self.torch_device, torch.int32).contiguous()
        if xy.dim() != 3 or xy.shape[2] != 2 or tuple(counts.shape) != (xy.shape[0],) or xy.shape[0] < 1 or xy.shape[1] < 1:
            raise ValueError("xy must be [sets,stride,2] and counts [sets]")
        perm = self._int32(*xy.shape[:2])
        self._call("fpc_cell_order", xy, counts, int(xy.shape[0]), int(xy.shape[1]), perm, inputs=(xy, counts))
        return perm

    def match_frames_guided_cells_async(self, n, H, radius, key=None, key_xy=None, pairing="key", cross_check=True,
                                        max_dist=0.0, ratio=0.0, stats=False):
        """fpc_match_frames_guided_cells: match_frames_guided_async's arguments and, bit for bit, its (match, dist), from
        the cell-ordered kernel that visits only the tiles the gate can reach.  stats=True: (match, dist, stats int32
        [n,2]: per frame (strip, tile) pairs visited, and the pairs there are).  Does not synchronise."""
        return self._guided_frames("_cells", stats, n, H, radius, key, key_xy, pairing, cross_check, max_dist, ratio)

    def match_frames_guided_cells(self, n, H, radius, key=None, key_xy=None, pairing="key", cross_check=True,
                                  max_dist=0.0, ratio=0.0):
        """match_frames_guided_cells_async, then per frame (match int32 [K_f], dist float32 [K_f])."""
        return self._per_frame(n, *self.match_frames_guided_cells_async(n, H, radius, key, key_xy, pairing, cross_check,
                                                                        max_dist, ratio))

    def match_bank_guided_cells_async(self, n, slot, H, radius, cross_check=True, max_dist=0.0, ratio=0.0, stats=False):
        """fpc_match_bank_guided_cells: match_bank_guided_async's arguments and, bit for bit, its (match, dist) on an
        "f32" bank (a "bf16" bank is refused); stats as in match_frames_guided_cells_async.  Does not synchronise."""
        return self._guided_bank("_cells", stats, n, slot, H, radius, cross_check, max_dist, ratio)

    def match_bank_guided_cells(self, n, slot, H, radius, cross_check=True, max_dist=0.0, ratio=0.0):
        """match_bank_guided_cells_async, then per frame (match int32 [K_f], dist float32 [K_f])."""
        return self._per_frame(n, *self.match_bank_guided_cells_async(n, slot, H, radius, cross_check, max_dist, ratio))

    # -- epipolar guided matching: the match once more under the estimated fundamental matrices (fpc_match_*_guided_epipolar)
    def match_frames_guided_epipolar_async(self, n, F, radius, key=None, key_xy=None, pairing="key", cross_check=True,
                                           max_dist=0.0, ratio=0.0):
        """fpc_match_frames_guided_epipolar: match_frames_guided_async's arguments with F (float32 [n,3,3] or [n,9], (u, v, 1)
        F (x, y, 1)^T = 0 for a query pixel (x, y) and its train pixel (u, v): fundamental_frames_async's output, device or
        host) in the place of H; the candidates of a row are the train rows within `radius` pixels (Sampson) of its epipolar
        line -> (match int32 [n,cap], dist float32 [n,cap]) on the device; a frame with F = 0 is all -1.  Does not
        synchronise."""
        return self._guided_frames("_epipolar", False, n, F, radius, key, key_xy, pairing, cross_check, max_dist, ratio)

    def match_frames_guided_epipolar(self, n, F, radius, key=None, key_xy=None, pairing="key", cross_check=True, max_dist=0.0,
                                     ratio=0.0):
        """match_frames_guided_epipolar_async, then per frame (match int32 [K_f], dist float32 [K_f])."""
        return self._per_frame(n, *self.match_frames_guided_epipolar_async(n, F, radius, key, key_xy, pairing, cross_check,
                                                                           max_dist, ratio))

    def match_bank_guided_epipolar_async(self, n, slot, F, radius, cross_check=True, max_dist=0.0, ratio=0.0):
        """fpc_match_bank_guided_epipolar: match_frames_guided_epipolar_async with frame f's train set taken from bank slot
        slot[f] (as match_bank_guided_async) and F fundamental_bank_async's output; an "f32" bank only (a "bf16" bank is
        refused).  Does not synchronise."""
        return self._guided_bank("_epipolar", False, n, slot, F, radius, cross_check, max_dist, ratio)

    def match_bank_guided_epipolar(self, n, slot, F, radius, cross_check=True, max_dist=0.0, ratio=0.0):
        """match_bank_guided_epipolar_async, then per frame (match int32 [K_f], dist float32 [K_f])."""
        return self._per_frame(n, *self.match_bank_guided_epipolar_async(n, slot, F, radius, cross_check, max_dist, ratio))

    # -- cell-ordered epipolar guided matching: the same tables, only the tiles the bands can reach
    # -- (fpc_match_*_guided_epipolar_cells)
    def match_frames_guided_epipolar_cells_async(self, n, F, radius, key=None, key_xy=None, pairing="key", cross_check=True,
                                                 max_dist=0.0, ratio=0.0, stats=False):
        """fpc_match_frames_guided_epipolar_cells: match_frames_guided_epipolar_async's arguments and, bit for bit, its
        (match, dist), from the cell-ordered kernel that visits only the tiles whose pixel box a row's epipolar band can
        reach.  stats=True: (match, dist, stats int32 [n,2]: per frame (strip, tile) pairs visited, and the pairs there
        are).  Does not synchronise."""
        return self._guided_frames("_epipolar_cells", stats, n, F, radius, key, key_xy, pairing, cross_check, max_dist, ratio)

    def match_frames_guided_epipolar_cells(self, n, F, radius, key=None, key_xy=None, pairing="key", cross_check=True,
                                           max_dist=0.0, ratio=0.0):
        """match_frames_guided_epipolar_cells_async, then per frame (match int32 [K_f], dist float32 [K_f])."""
        return self._per_frame(n, *self.match_frames_guided_epipolar_cells_async(n, F, radius, key, key_xy, pairing,
                                                                                 cross_check, max_dist, ratio))

    def match_bank_guided_epipolar_cells_async(self, n, slot, F, radius, cross_check=True, max_dist=0.0, ratio=0.0,
                                               stats=False):
        """fpc_match_bank_guided_epipolar_cells: match_bank_guided_epipolar_async's arguments and, bit for bit, its (match,
        dist) on an "f32" bank (a "bf16" bank is refused); stats as in match_frames_guided_epipolar_cells_async.  Does not
        synchronise."""
        return self._guided_bank("_epipolar_cells", stats, n, slot, F, radius, cross_check, max_dist, ratio)

    def match_bank_guided_epipolar_cells(self, n, slot, F, radius, cross_check=True, max_dist=0.0, ratio=0.0):
        """match_bank_guided_epipolar_cells_async, then per frame (match int32 [K_f], dist float32 [K_f])."""
        return self._per_frame(n, *self.match_bank_guided_epipolar_cells_async(n, slot, F, radius, cross_check, max_dist,
                                                                               ratio))

    # -- pose-guided matching: the match once more under the estimated absolute poses, "search by projection"
    # -- (fpc_match_*_guided_pose)
    def _guided_pose(self, name, n, train, R, t, radius, K, cross_check, max_dist, ratio):
        """fpc_<name>(ctx, n, *train, R, t, fx, fy, cx, cy, radius, ...): what both pose-guided calls do behind their
        train set's checks."""
        rm = self._guided_h(n, R, "R")
        tv = torch.as_tensor(t).to(self.torch_device, torch.float32).contiguous()
        if tuple(tv.shape) != (n, 3):
            raise ValueError("t must be [n,3]")
        p = self._pnp_params(K, {})
        m, d = self._table(n)
        self._call(name, n, *train, rm, tv, float(p.fx), float(p.fy), float(p.cx), float(p.cy), float(radius),
                   int(bool(cross_check)), float(max_dist), float(ratio), m, d, inputs=(*train, rm, tv))
        return m, d

    def match_frames_guided_pose_async(self, n, R, t, radius, key, key_xyz, key_valid=None, K=None, cross_check=True,
                                       max_dist=0.0, ratio=0.0):
        """fpc_match_frames_guided_pose: match_frames_async against `key` over the key rows whose 3-D point -- key_xyz /
        key_valid as in pnp_frames_async -- projects within `radius` pixels of the query row under the frame's pose: R
        (float32 [n,3,3] or [n,9]) and t (float32 [n,3]) with X_cam = R X + t, pnp_frames_async's output, device or
        host.  K: the camera as in ransac_pnp_async -> (match int32 [n,cap], dist float32 [n,cap]) on the device; a frame
        with R = t = 0 is all -1.  Does not synchronise."""
        kd, kc = self._key(key)
        if kd is None:
            raise ValueError("the pose-guided match needs a key")
        kx, kv, _ = self._key_landmarks(key_xyz, key_valid)
        if kx.shape[0] < kd.shape[0]:
            raise ValueError("a key needs key_xyz with a row for each of its rows")
        return self._guided_pose("fpc_match_frames_guided_pose", n, (kd, kc, kx, kv), R, t, radius, K, cross_check,
                                 max_dist, ratio)

    def match_frames_guided_pose(self, n, R, t, radius, key, key_xyz, key_valid=None, K=None, cross_check=True,
                                 max_dist=0.0, ratio=0.0):
        """match_frames_guided_pose_async, then per frame (match int32 [K_f], dist float32 [K_f])."""
        return self._per_frame(n, *self.match_frames_guided_pose_async(n, R, t, radius, key, key_xyz, key_valid, K,
                                                                       cross_check, max_dist, ratio))

    def match_bank_guided_pose_async(self, n, slot, R, t, radius, K=None, cross_check=True, max_dist=0.0, ratio=0.0):
        """fpc_match_bank_guided_pose: match_frames_guided_pose_async with frame f's train set and landmarks taken from bank
        slot slot[f] (as match_bank_guided_async) and R, t pnp_bank_async's output; an "f32" bank only (a "bf16" bank is
        refused); a bank without landmarks gives all -1.  Does not synchronise."""
        self._bank_info()
        slot = self._dev_int32("slot", slot, "[n]", n)
        return self._guided_pose("fpc_match_bank_guided_pose", n, (slot,), R, t, radius, K, cross_check, max_dist, ratio)

    def match_bank_guided_pose(self, n, slot, R, t, radius, K=None, cross_check=True, max_dist=0.0, ratio=0.0):
        """match_bank_guided_pose_async, then per frame (match int32 [K_f], dist float32 [K_f])."""
        return self._per_frame(n, *self.match_bank_guided_pose_async(n, slot, R, t, radius, K, cross_check, max_dist,
                                                                     ratio))

    # -- timing ----------------------------------------------------------------------
    def check_guards(self):
        """Contexts created with plan_flags=["guard_zones"] (a test facility): waits for the device and returns the number
        of 32-bit words of the workspace's canary zones that a kernel has overwritten (0 = every store stayed inside
        its tensor)."""
        bad = ctypes.c_longlong(0)
        _lib.check(self._l.fpc_check_guards(self._ctx, ctypes.byref(bad)), "fpc_check_guards")
        return int(bad.value)

    def set_timing(self, on):
        """on = True / False, or an int n > 1: only every n-th detect call (the first included) carries the events."""
        _lib.check(self._l.fpc_set_timing(self._ctx, int(on) if on is not True else 1), "fpc_set_timing")

    def timings(self):
        """[(layer name, kernel symbol, ms, algorithmic FLOPs, MFMA-issued FLOPs, algorithmic HBM bytes)] of the
        launches recorded since set_timing(True) (FLOPs and bytes are per LAUNCH: per frame x the launch's frames)."""
        cap = max(128, _lib.check(self._l.fpc_get_timings(self._ctx, 0, None, None, None, None, None, None), "fpc_get_timings"))
        names = (ctypes.c_char_p * cap)()
        kernels = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_float * cap)()
        fl = (ctypes.c_double * cap)()
        mf = (ctypes.c_double * cap)()
        by = (ctypes.c_double * cap)()
        n = _lib.check(self._l.fpc_get_timings(self._ctx, cap, names, kernels, ms, fl, mf, by), "fpc_get_timings")
        return [(names[i].decode(), kernels[i].decode(), float(ms[i]), float(fl[i]), float(mf[i]), float(by[i]))
                for i in range(min(n, cap))]


    def kernel_names(self, frames):
        """Kernel symbols one fpc_forward over `frames` launches (through the timing facility: events on, one call, events off)."""
        self.set_timing(True)
        self.forward(frames)
        self.sync()
        out = [k for _, k, _, _, _, _ in self.timings()]
        self.set_timing(False)
        return out


def _ptr(a):
    """A tensor's device pointer; anything else (None, a host scalar, a ctypes reference) as it is."""
    return a.data_ptr() if isinstance(a, torch.Tensor) else a


class _DevArray:
    """Minimal __cuda_array_interface__ holder so torch can alias library-owned memory."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def conv_flops_per_frame(h, w, descriptor=True):
    return 2.0 * arch.conv_macs(h, w, descriptor)
