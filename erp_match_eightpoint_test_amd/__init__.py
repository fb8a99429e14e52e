"""MI355X-native ERP matcher + spherical eight-point estimator.

Host-side mirror of the reference's hot-path classes (Kitsunetic/ERP_match_eightpoint_test):

* ``feature_matcher.match_two_image``  -- src/feature_matcher.cpp:42-59
* ``eight_point.find / initial_guess / eight_point_estimation`` -- src/eight_point.cpp:16-192
* ``erp_rotation`` / ``spherical_surf`` -- the ERP remaps either side of the path
  (src/erp_rotation.cpp:14-122, src/spherical_surf.cpp:16-133, src/automatic.cpp:50-79,148-152)
* ``epipolar_tool`` / ``feature_matcher.draw_match`` -- the visual outputs
  (src/epipolar_tool.cpp:7-128, src/feature_matcher.cpp:61-86)
* ``PairBatchRunner`` -- the batched hot path: match -> gather -> find for many ERP pairs,
  i.e. what src/automatic.cpp:117-126 runs per pair, as one sequence of gfx950 kernels
  (``run`` from descriptors, ``run_images`` from the ERP images via
  ``spherical_surf.do_all_batch``, ``run_sweep`` for the drivers' rotation sweeps: one left
  image against a right base image under a list of poses, with the surf match error,
  ``rectify_images`` on to automatic's rectified and vertical views of every pair).
* ``stereo`` -- dense disparity and depth on those vertical views (census + 4- or 8-path SGM; no
  reference counterpart, include/erp_match.h "dense stereo on row-rectified views").

Every call goes through the C ABI of ``lib/liberp_match.so`` (include/erp_match.h); there is
no CPU fallback.  Arrays are numpy (host, synchronous) or torch CUDA tensors (device,
asynchronous on torch's current stream).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi, synth
from .capi import (DMATCH_DTYPE, HYP_DTYPE, POLISH_DTYPE, POLISH_ROUND_DTYPE, POSE_DTYPE, RESULT_DTYPE,
                   SUPPORT_DTYPE, WINNER_DTYPE, Context, ErpError, RandStream, check, default_cfg,
                   process_rand_stream, support_to_numpy)

__all__ = ["feature_matcher", "eight_point", "erp_rotation", "spherical_surf", "epipolar_tool",
           "PairBatchRunner", "Context", "ErpError", "RandStream", "process_rand_stream",
           "default_cfg", "DMATCH_DTYPE", "HYP_DTYPE", "RESULT_DTYPE", "POLISH_DTYPE",
           "POLISH_ROUND_DTYPE", "WINNER_DTYPE", "results_to_numpy", "hyps_to_numpy",
           "polish_to_numpy", "polish_rounds_to_numpy", "winners_to_numpy", "sweep_relative_rotation", "synth", "capi",
           "POSE_DTYPE", "pose_to_numpy", "SUPPORT_DTYPE", "support_to_numpy", "stereo"]


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class feature_matcher:  # noqa: N801  (reference class name)
    """feature_matcher (src/feature_matcher.hpp:26-51), hot-path subset.

    match_two_image(descriptor1, descriptor2) -> structured array of DMatch
    (queryIdx, trainIdx, imgIdx, distance), ascending queryIdx, kept when d0 < 0.3 * d1.
    """

    def __init__(self, device: int = 0, ctx: Context | None = None, method: int | None = None):
        self.ctx = ctx or Context(device)
        if method is not None:  # capi.MATCHER_MFMA_FILTER (default) / capi.MATCHER_VALU_EXACT
            self.ctx.set_matcher(method)

    def match_two_image(self, descriptor1, descriptor2, ratio: float = 0.3):
        try:
            import torch
            is_torch = isinstance(descriptor1, torch.Tensor)
        except ImportError:  # pragma: no cover
            is_torch = False
        if is_torch:
            return self._match_device(descriptor1, descriptor2, ratio)
        q = np.ascontiguousarray(descriptor1, np.float32)
        t = np.ascontiguousarray(descriptor2, np.float32)
        if q.ndim != 2 or t.ndim != 2 or q.shape[1] != t.shape[1]:
            raise ValueError("descriptors must be 2-D with equal columns")
        if abs(ratio - 0.3) > 0:
            tq = self._to_device(q)
            tt = self._to_device(t)
            return self._match_device(tq, tt, ratio).cpu().numpy().view(DMATCH_DTYPE).reshape(-1)
        out = np.zeros(max(q.shape[0], 1), DMATCH_DTYPE)
        n = C.c_int32(0)
        check(self.ctx.L.erp_match_two_image(self.ctx.h, _np_ptr(q), q.shape[0], _np_ptr(t),
                                             t.shape[0], q.shape[1], _np_ptr(out), C.byref(n)),
              "match_two_image")
        return out[:n.value].copy()

    def match_guided(self, descriptor1, descriptor2, key1, key2, im_width: int, im_height: int,
                     E, thr: float = 0.003, ratio: float = 0.8, max_dist: float = 0.0,
                     unique: bool = True):
        """Guided matching (include/erp_match.h "guided matching"; no reference counterpart):
        descriptor1 rows rematched among the descriptor2 rows whose keypoint lies in the
        epipolar band |l^T E' r| < thr of the solved 9-vector E (E' its rank-2 correction), kept
        when d0 < ratio * d1 inside the band (and d0 < max_dist when max_dist > 0; ``unique``:
        one query per train row) -> DMatch array, ascending queryIdx.  Host arrays, one pair,
        synchronous (erp_match_guided)."""
        q = np.ascontiguousarray(descriptor1, np.float32)
        t = np.ascontiguousarray(descriptor2, np.float32)
        k1, k2 = _keys_host(key1), _keys_host(key2)
        e = np.ascontiguousarray(E, np.float64).reshape(-1)
        if q.ndim != 2 or t.ndim != 2 or q.shape[1] != 64 or t.shape[1] != 64 or \
                len(k1) != q.shape[0] or len(k2) != t.shape[0] or e.size != 9:
            raise ValueError("match_guided: descriptors [n, 64] with one keypoint per row and a "
                             "9-element E expected")
        out = np.zeros(max(q.shape[0], 1), DMATCH_DTYPE)
        n = C.c_int32(0)
        cfg = capi.GuidedCfg(thr, ratio, max_dist, 1 if unique else 0)
        check(self.ctx.L.erp_match_guided(self.ctx.h, _np_ptr(q), q.shape[0], _np_ptr(t),
                                          t.shape[0], _np_ptr(k1), _np_ptr(k2), im_width,
                                          im_height, _np_ptr(e), C.byref(cfg), _np_ptr(out),
                                          C.byref(n)), "match_guided")
        return out[:n.value].copy()

    # ---- SURF (src/feature_matcher.cpp:26-40, xfeatures2d::SURF::create() defaults) ----
    def surf(self, images, max_kp: int = 16384, **params):
        """detect_key_point + comput_descriptor on CUDA uint8 images [n, H, W] (gray) or
        [n, H, W, 3] (BGR); a single [H, W] / [H, W, 3] image is one image -> (keypoints list
        of KEYPOINT_DTYPE arrays, descriptor list of [k, 64] float32), per image, in OpenCV's
        KeypointGreater order.  Parity with OpenCV is unpinned (oracle/erp_surf.c)."""
        kp, desc, counts = self.surf_dev(images, max_kp, **params)
        c = int(counts.max()) if len(counts) else 0
        kps = kp[:, :c].cpu().numpy()
        ds = desc[:, :c].cpu().numpy()
        return ([kps[i, :counts[i]].reshape(-1).view(capi.KEYPOINT_DTYPE).copy()
                 for i in range(len(counts))],
                [ds[i, :counts[i]].copy() for i in range(len(counts))])

    def surf_dev(self, images, max_kp: int = 16384, **params):
        """surf() without leaving the device -> (keypoints uint8 [n, max_kp', 28] (view as
        float32 [.., 7]: x, y, size, angle, response, octave, class_id), descriptors float32
        [n, max_kp', 64], counts numpy int32 [n]); rows [0, counts[i]) of image i are valid.
        max_kp' >= max_kp grows when an image overflows (the call is repeated)."""
        import torch
        if images.dim() == 2 or (images.dim() == 3 and images.shape[-1] == 3):
            images = images.unsqueeze(0)  # one gray [H, W] or one BGR [H, W, 3] image
        if not (images.is_cuda and images.dtype == torch.uint8 and images.is_contiguous()):
            raise ValueError("images must be contiguous CUDA uint8 tensors")
        ch = 3 if images.dim() == 4 else 1
        n, H, W = images.shape[:3]
        prm = capi.SurfParams()
        self.ctx.L.erp_surf_params_default(C.byref(prm))
        for k, v in params.items():
            setattr(prm, k, v)
        st = torch.cuda.current_stream(images.device).cuda_stream
        while True:
            kp = torch.empty((n, max_kp, 28), dtype=torch.uint8, device=images.device)
            desc = torch.empty((n, max_kp, 64), dtype=torch.float32, device=images.device)
            cnt = torch.zeros(n, dtype=torch.int32, device=images.device)
            check(self.ctx.L.erp_surf_detect_compute_dev(self.ctx.h, images.data_ptr(), n, W, H, ch,
                                                         C.byref(prm), max_kp, kp.data_ptr(),
                                                         desc.data_ptr(), cnt.data_ptr(), st),
                  "erp_surf_detect_compute_dev")
            counts = cnt.cpu().numpy()
            if (counts >= 0).all():
                return kp, desc, counts
            max_kp = int(-counts.min()) + 16

    def draw_match(self, im_left, im_right, key_left, key_right):
        """draw_match (src/feature_matcher.cpp:61-86): CUDA uint8 BGR images [H, W, 3] and the
        matched keypoints (CUDA float32 [M, 2] or anything array-like of (pt.x, pt.y)) -> the
        overlay [H, W, 3]: grey left / right in channels 0 / 1, a 5-px line per match coloured
        HSV(i 180 / M, 180, 150), later matches on top."""
        import torch
        im_left, im_right = _img_dev(im_left), _img_dev(im_right)
        if im_left.shape != im_right.shape:
            raise ValueError("draw_match: the two images differ in size")
        if im_left.device != im_right.device or im_left.device.index != self.ctx.device:
            raise ValueError(f"draw_match: images must be on the context's device "
                             f"cuda:{self.ctx.device}")
        H, W = im_left.shape[:2]
        kl, kr = _keys_dev(key_left, im_left.device), _keys_dev(key_right, im_left.device)
        m = min(kl.shape[0], kr.shape[0])
        if kl.shape[0] != kr.shape[0]:
            raise ValueError("draw_match: key_left and key_right differ in length")
        out = torch.empty_like(im_left)
        check(self.ctx.L.erp_draw_match_dev(self.ctx.h, im_left.data_ptr(), im_right.data_ptr(),
                                            W, H, kl.data_ptr() if m else None,
                                            kr.data_ptr() if m else None, m, out.data_ptr(),
                                            torch.cuda.current_stream(im_left.device).cuda_stream),
              "draw_match")
        return out

    def _to_device(self, a):
        import torch
        return torch.from_numpy(a).to(f"cuda:{self.ctx.device}")

    def _match_device(self, q, t, ratio):
        """device path: torch float32 CUDA tensors -> torch int32 tensor [M, 4] (DMatch rows)."""
        import torch
        q = q.contiguous()
        t = t.contiguous()
        assert q.dtype == torch.float32 and t.dtype == torch.float32 and q.is_cuda and t.is_cuda
        out = torch.empty((max(q.shape[0], 1), 4), dtype=torch.int32, device=q.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=q.device)
        st = torch.cuda.current_stream(q.device).cuda_stream
        check(self.ctx.L.erp_match_knn2_ratio(self.ctx.h, q.data_ptr(), q.shape[0], t.data_ptr(),
                                              t.shape[0], q.shape[1], ratio, out.data_ptr(),
                                              cnt.data_ptr(), st), "match_knn2_ratio")
        return out[: int(cnt.item())]


def _keys(key_left, key_right, match_size):
    """-> (kl, kr, m): the first m = match_size (None: all of key_left) keypoints of each side
    as contiguous float32 [m, 2]"""
    kl = np.ascontiguousarray(key_left, np.float32).reshape(-1, 2)
    kr = np.ascontiguousarray(key_right, np.float32).reshape(-1, 2)
    m = kl.shape[0] if match_size is None else int(match_size)
    if m > kl.shape[0] or m > kr.shape[0]:
        raise ValueError("match_size larger than the keypoint arrays")
    return np.ascontiguousarray(kl[:m]), np.ascontiguousarray(kr[:m]), m


def _support_thr(thr) -> float:
    """the support stage's threshold as the C float: finite and > 0, checked before any call"""
    if thr is None:
        raise ValueError("the support stage needs a threshold (support_thr / thr > 0)")
    t = float(np.float32(thr))
    if not (np.isfinite(t) and t > 0.0):
        raise ValueError(f"support threshold must be finite and > 0, got {thr!r}")
    return t


def _record(struct, dtype):
    """a ctypes record as a numpy scalar of its structured dtype"""
    return np.frombuffer(bytes(struct), dtype)[0]


class eight_point:  # noqa: N801  (reference class name)
    """eight_point (src/eight_point.hpp:8-28).  ``cfg`` holds the reference constants.
    ``stream``: a RandStream that find / initial_guess draw from and advance, as the reference's
    finds share the process-global rand() (``stream=process_rand_stream()``); the default,
    None, starts every call at cfg.seed / cfg.offset."""

    def __init__(self, device: int = 0, ctx: Context | None = None,
                 stream: RandStream | None = None, **cfg):
        self.ctx = ctx or Context(device)
        self.cfg = default_cfg(**cfg)
        self.last_result = None
        self.last_polish = None
        self.last_winner = None
        self.last_pose = None
        self.last_support = None
        self.last_support_result = None
        self.last_counts = None
        if stream is not None:
            self.ctx.set_rand_stream(stream)

    def find(self, im_width: int, im_height: int, key_left, key_right, match_size: int | None = None):
        """-> (R_vec_out (3,) float32, T_vec_out (3,) float32); raises ErpError on the
        reference's undefined-behaviour cases (too few points, no valid hypothesis)."""
        kl, kr, m = _keys(key_left, key_right, match_size)
        R = np.zeros(3, np.float32)
        T = np.zeros(3, np.float32)
        res = capi.PairResult()
        st = self.ctx.L.erp_eight_point_find(self.ctx.h, im_width, im_height, _np_ptr(kl),
                                             _np_ptr(kr), m, C.byref(self.cfg), _np_ptr(R),
                                             _np_ptr(T), C.byref(res))
        self.last_result = _record(res, RESULT_DTYPE)
        check(st, "find")
        return R, T

    def find_winner(self, im_width: int, im_height: int, key_left, key_right,
                    match_size: int | None = None):
        """find plus the winning iteration's essential matrix (erp_eight_point_find_winner; no
        reference counterpart) -> (R (3,), T (3,), E (3, 3) float64): E is the solved 9-vector
        R and T were decomposed from (sign arbitrary), e.g. for epipolar_tool.draw_epipole.
        ``last_winner`` is the record (WINNER_DTYPE: status, iter, which, sample_n, E)."""
        kl, kr, m = _keys(key_left, key_right, match_size)
        R = np.zeros(3, np.float32)
        T = np.zeros(3, np.float32)
        res, win = capi.PairResult(), capi.Winner()
        st = self.ctx.L.erp_eight_point_find_winner(self.ctx.h, im_width, im_height, _np_ptr(kl),
                                                    _np_ptr(kr), m, C.byref(self.cfg), _np_ptr(R),
                                                    _np_ptr(T), C.byref(res), C.byref(win))
        self.last_result = _record(res, RESULT_DTYPE)
        self.last_winner = _record(win, WINNER_DTYPE)
        check(st, "find_winner")
        check(int(self.last_winner["status"]), "find_winner: winner record")
        return R, T, self.last_winner["E"].reshape(3, 3).copy()

    def find_support(self, im_width: int, im_height: int, key_left, key_right, thr: float,
                     match_size: int | None = None, want_counts: bool = False):
        """find plus the support stage (erp_eight_point_find_support; no reference counterpart)
        -> (R (3,), T (3,), E (3, 3) float64) of the scored iteration that most matches agree
        with under |l^T E' r| < thr (the first such iteration on ties), instead of the consensus
        winner find returns.  It pays with minimal samples (``sample_frac`` chosen for about 10
        rows), not at the reference's 0.25.  ``last_result`` is find's own
        record, ``last_support`` the support record (SUPPORT_DTYPE: status, iter, which, inliers,
        scored, consensus_iter, consensus_inliers, row), ``last_winner`` that iteration's winner
        record, ``last_support_result`` find's record with R, T and min_idx replaced, and
        ``last_counts`` (want_counts) every iteration's inlier count.  Consumes a rand stream
        exactly as find does."""
        thr = _support_thr(thr)
        kl, kr, m = _keys(key_left, key_right, match_size)
        R = np.zeros(3, np.float32)
        T = np.zeros(3, np.float32)
        res, sres = capi.PairResult(), capi.PairResult()
        sup, win = capi.Support(), capi.Winner()
        counts = np.zeros(max(self.cfg.iters, 1), np.int32) if want_counts else None
        st = self.ctx.L.erp_eight_point_find_support(
            self.ctx.h, im_width, im_height, _np_ptr(kl), _np_ptr(kr), m, C.byref(self.cfg), thr,
            _np_ptr(R), _np_ptr(T), C.byref(res), C.byref(sup), C.byref(win), C.byref(sres),
            _np_ptr(counts) if want_counts else None)
        self.last_result = _record(res, RESULT_DTYPE)
        self.last_support = _record(sup, SUPPORT_DTYPE)
        self.last_winner = _record(win, WINNER_DTYPE)
        self.last_support_result = _record(sres, RESULT_DTYPE)
        self.last_counts = counts[:self.cfg.iters] if want_counts else None
        check(st, "find_support")
        check(int(self.last_support["status"]), "find_support: support record")
        return R, T, self.last_winner["E"].reshape(3, 3).copy()

    def find_polished(self, im_width: int, im_height: int, key_left, key_right, thr: float,
                      rounds: int = 3, match_size: int | None = None):
        """find followed by the polish stage (erp_eight_point_find_polished; no reference
        counterpart): the winner's inliers under |l^T E' r| < thr and up to ``rounds`` refits on
        them -> (R (3,), T (3,), inlier_mask (match_size,) bool) of the last accepted state.
        ``last_result`` is find's record (its R, T are find's answer), ``last_polish`` the
        polish record (POLISH_DTYPE).  Consumes a rand stream exactly as find does."""
        kl, kr, m = _keys(key_left, key_right, match_size)
        res, pol = capi.PairResult(), capi.PolishResult()
        mask = np.zeros(max(m, 1), np.uint8)
        st = self.ctx.L.erp_eight_point_find_polished(self.ctx.h, im_width, im_height, _np_ptr(kl),
                                                      _np_ptr(kr), m, C.byref(self.cfg), thr,
                                                      int(rounds), C.byref(res), C.byref(pol),
                                                      _np_ptr(mask))
        self.last_result = _record(res, RESULT_DTYPE)
        self.last_polish = _record(pol, POLISH_DTYPE)
        check(st, "find_polished")
        return self.last_polish["R"].copy(), self.last_polish["T"].copy(), mask[:m].astype(bool)

    def find_posed(self, im_width: int, im_height: int, key_left, key_right, thr: float,
                   rounds: int = 3, min_sin2: float = 0.0, match_size: int | None = None):
        """find, the polish and the pose selection (erp_eight_point_find_posed; no reference
        counterpart): the cheirality vote over (R1 | R2) x (+t | -t) on the polish's E and inlier
        set -> (R (3,), T (3,), inlier_mask (match_size,) bool, depth (match_size, 2) float64,
        front (match_size,) bool).  R, T are the pose record's: the reference's candidates made
        definite.  ``last_result`` is find's record, ``last_polish`` the polish's, ``last_pose``
        the pose record (POSE_DTYPE; its status is ERP_TOO_FEW_POINTS when no match could vote).
        Consumes a rand stream exactly as find does."""
        kl, kr, m = _keys(key_left, key_right, match_size)
        res, pol, pose = capi.PairResult(), capi.PolishResult(), capi.Pose()
        mask = np.zeros(max(m, 1), np.uint8)
        front = np.zeros(max(m, 1), np.uint8)
        depth = np.zeros((max(m, 1), 2), np.float64)
        st = self.ctx.L.erp_eight_point_find_posed(self.ctx.h, im_width, im_height, _np_ptr(kl),
                                                   _np_ptr(kr), m, C.byref(self.cfg), thr,
                                                   int(rounds), float(min_sin2), C.byref(res),
                                                   C.byref(pol), C.byref(pose), _np_ptr(mask),
                                                   _np_ptr(depth), _np_ptr(front))
        self.last_result = _record(res, RESULT_DTYPE)
        self.last_polish = _record(pol, POLISH_DTYPE)
        self.last_pose = _record(pose, POSE_DTYPE)
        check(st, "find_posed")
        return (self.last_pose["R"].copy(), self.last_pose["T"].copy(), mask[:m].astype(bool),
                depth[:m], front[:m].astype(bool))

    def initial_guess(self, im_width: int, im_height: int, key_point_left_rect,
                      key_point_right_rect, match_size: int | None = None):
        bl = np.ascontiguousarray(key_point_left_rect, np.float64).reshape(-1, 3)
        br = np.ascontiguousarray(key_point_right_rect, np.float64).reshape(-1, 3)
        m = bl.shape[0] if match_size is None else int(match_size)
        R = np.zeros(3, np.float32)
        T = np.zeros(3, np.float32)
        res = capi.PairResult()
        st = self.ctx.L.erp_initial_guess(self.ctx.h, _np_ptr(bl), _np_ptr(br), m,
                                          C.byref(self.cfg), _np_ptr(R), _np_ptr(T), C.byref(res))
        self.last_result = _record(res, RESULT_DTYPE)
        check(st, "initial_guess")
        return R, T

    def eight_point_estimation(self, im_width: int, im_height: int, key_point_left_rect,
                               key_point_right_rect, match_size: int | None = None):
        """-> (R1_vec, R2_vec, T_vec, R1_valid, R2_valid, E)"""
        bl = np.ascontiguousarray(key_point_left_rect, np.float64).reshape(-1, 3)
        br = np.ascontiguousarray(key_point_right_rect, np.float64).reshape(-1, 3)
        m = bl.shape[0] if match_size is None else int(match_size)
        h = capi.Hypothesis()
        check(self.ctx.L.erp_eight_point_estimation(self.ctx.h, _np_ptr(bl), _np_ptr(br), m,
                                                    C.byref(h)), "eight_point_estimation")
        r = _record(h, HYP_DTYPE)
        return (r["R1"].copy(), r["R2"].copy(), r["T"].copy(), bool(r["R1_valid"]),
                bool(r["R2_valid"]), r["E"].copy())


def _keys_dev(k, device):
    """(pt.x, pt.y) rows as a contiguous CUDA float32 tensor [n, 2]"""
    import torch
    if isinstance(k, torch.Tensor):
        t = k.to(device=device, dtype=torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(k, np.float32)).to(device)
    return t.reshape(-1, 2).contiguous()


def _keys_host(k) -> np.ndarray:
    try:
        import torch
        if isinstance(k, torch.Tensor):
            k = k.detach().cpu().numpy()
    except ImportError:  # pragma: no cover
        pass
    return np.ascontiguousarray(k, np.float32).reshape(-1, 2)


class epipolar_tool:  # noqa: N801  (reference class name)
    """epipolar_tool (src/epipolar_tool.hpp:7-31, .cpp:7-128): picks test_key_num (<= 7) of the
    matched pairs with std::random_shuffle on the glibc rand() stream -- (seed, offset) = the
    process-global rand() state, (1, 0) in a fresh process -- and draws, for an essential
    matrix, the epipolar curves of their left keypoints and dots at their right keypoints on an
    output_width x output_height ERP canvas (a CUDA uint8 tensor [H, W, 3])."""

    def __init__(self, left_key, right_key, im_width: int, im_height: int, output_width: int,
                 output_height: int, test_key_num: int, seed: int = 1, offset: int = 0,
                 device: int = 0, ctx: Context | None = None, stream: RandStream | None = None):
        """stream: the constructor's shuffle draws from this RandStream and advances it by
        match_size - 1 (seed / offset are then the stream's position at that moment)"""
        self.ctx = ctx or Context(device)
        self.left_key, self.right_key = _keys_host(left_key), _keys_host(right_key)
        if self.left_key.shape != self.right_key.shape:
            raise ValueError("epipolar_tool: left_key and right_key differ in length")
        self.match_size = self.left_key.shape[0]
        self.n_key = int(test_key_num)
        self.im_width, self.im_height = int(im_width), int(im_height)
        self.epipole_mat_width, self.epipole_mat_height = int(output_width), int(output_height)
        self.seed, self.offset = int(seed), int(offset)
        if not (1 <= self.match_size and 0 <= self.n_key <= min(7, self.match_size)):
            raise ErpError(capi.ERP_INVALID_ARG,
                           "epipolar_tool: need 0 <= test_key_num <= min(7, match_size)")
        # the constructor's choice (src/epipolar_tool.cpp:13-16), available before any draw
        if stream is not None:
            self.seed, self.offset = stream.get()
            self.random_idx = stream.shuffle_prefix(self.match_size, self.n_key)
            return
        self.random_idx = np.zeros(self.n_key, np.int32)
        check(self.ctx.L.erp_random_shuffle_prefix(self.seed, self.offset, self.match_size,
                                                   self.n_key, _np_ptr(self.random_idx)),
              "random_shuffle_prefix")

    def draw_epipole(self, test_E_mat):  # noqa: N803  (reference argument name)
        import torch
        E = _m9(test_E_mat)
        dev = torch.device(f"cuda:{self.ctx.device}")
        out = torch.empty((self.epipole_mat_height, self.epipole_mat_width, 3), dtype=torch.uint8,
                          device=dev)
        # the draw repeats the constructor's choice at its recorded (seed, offset): a rand
        # stream attached to the context must not be consumed a second time
        attached = self.ctx.rand_stream
        if attached is not None:
            self.ctx.set_rand_stream(None)
        try:
            return self._draw(E, out, dev)
        finally:
            if attached is not None:
                self.ctx.set_rand_stream(attached)

    def _draw(self, E, out, dev):
        import torch
        check(self.ctx.L.erp_epipolar_draw_dev(
            self.ctx.h, _np_ptr(self.left_key), _np_ptr(self.right_key), self.match_size,
            self.im_width, self.im_height, self.epipole_mat_width, self.epipole_mat_height,
            self.n_key, self.seed, self.offset, _np_ptr(E), out.data_ptr(),
            _np_ptr(self.random_idx), torch.cuda.current_stream(dev).cuda_stream), "draw_epipole")
        return out


def _m9(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).reshape(9)


def _img_dev(im):
    import torch
    if not (isinstance(im, torch.Tensor) and im.is_cuda and im.dtype == torch.uint8
            and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous()):
        raise ValueError("images are contiguous CUDA uint8 tensors [H, W, 3] (CV_8UC3)")
    return im


class erp_rotation:  # noqa: N801  (reference class name)
    """erp_rotation (src/erp_rotation.hpp:9-19).  Matrices are host numpy (3, 3) float64;
    images are CUDA uint8 tensors [H, W, 3].  Output pixels whose source falls outside the
    image are not written (uninitialised in the reference): ``fill`` pre-fills them."""

    def __init__(self, device: int = 0, ctx: Context | None = None):
        self.ctx = ctx or Context(device)
        self.L = self.ctx.L

    def eular2rot(self, theta) -> np.ndarray:
        th = np.ascontiguousarray(theta, np.float64).reshape(3)
        R = np.zeros(9, np.float64)
        self.L.erp_eular2rot(_np_ptr(th), _np_ptr(R))
        return R.reshape(3, 3)

    def rot2eular(self, R) -> np.ndarray:
        m = _m9(R)
        e = np.zeros(3, np.float64)
        self.L.erp_rot2eular(_np_ptr(m), _np_ptr(e))
        return e

    def rotate_image(self, im, rot_mat, fill: int = 0):
        import torch
        im = _img_dev(im)
        H, W = im.shape[:2]
        out = torch.full_like(im, fill)
        m = _m9(rot_mat)
        check(self.L.erp_rotate_image_dev(self.ctx.h, im.data_ptr(), W, H, _np_ptr(m),
                                          out.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "rotate_image")
        return out

    def match_error(self, key_left, key_right, counts, rot_mats, W: int, H: int):
        """erp_match_error_dev, the "Surf match error" of one_image_test/main.cpp:115-129: per
        pair the mean over its matches of degree_error(rotate_pixel(key_left, rot_mat),
        key_right), radians.  key_left / key_right: CUDA float32 [P, S, 2] (pair p's matches in
        its first counts[p] of S slots); counts: CUDA int32 [P], any stride (e.g. the M column of
        a batch's records); rot_mats: host [P, 3, 3] -> CUDA float64 [P], NaN where counts is 0."""
        import torch
        mats = _rot_mats_host(rot_mats)
        for k in (key_left, key_right):
            if not (isinstance(k, torch.Tensor) and k.is_cuda and k.dtype == torch.float32
                    and k.dim() == 3 and k.shape[2] == 2 and k.is_contiguous()):
                raise ValueError("keys are contiguous CUDA float32 tensors [P, S, 2]")
        if not (isinstance(counts, torch.Tensor) and counts.is_cuda and counts.dtype == torch.int32
                and counts.dim() == 1 and (counts.shape[0] < 2 or counts.stride(0) >= 1)):
            raise ValueError("counts is a CUDA int32 tensor [P]")
        P_, S = key_left.shape[:2]
        if key_right.shape != key_left.shape or counts.shape[0] != P_ or mats.shape[0] != P_:
            raise ValueError("key_left, key_right, counts and rot_mats differ in pair count")
        if not (key_left.device == key_right.device == counts.device
                and key_left.device.index == self.ctx.device):
            raise ValueError(f"tensors must be on the context's device cuda:{self.ctx.device}")
        out = torch.empty(P_, dtype=torch.float64, device=key_left.device)
        check(self.L.erp_match_error_dev(self.ctx.h, key_left.data_ptr(), key_right.data_ptr(), S,
                                         counts.data_ptr(),
                                         counts.stride(0) if P_ > 1 else 1, P_, _np_ptr(mats),
                                         int(W), int(H), out.data_ptr(),
                                         torch.cuda.current_stream(key_left.device).cuda_stream),
              "erp_match_error_dev")
        return out

    def rot_from_vec(self, v1, v2) -> np.ndarray:
        a = np.ascontiguousarray(v1, np.float64).reshape(3)
        b = np.ascontiguousarray(v2, np.float64).reshape(3)
        R = np.zeros(9, np.float64)
        self.L.erp_rot_from_vec(_np_ptr(a), _np_ptr(b), _np_ptr(R))
        return R.reshape(3, 3)

    def inv(self, m) -> np.ndarray:
        """cv::Mat::inv() of a 3x3 double matrix"""
        a = _m9(m)
        o = np.zeros(9, np.float64)
        if not self.L.erp_inv3(_np_ptr(a), _np_ptr(o)):
            raise ErpError(capi.ERP_INVALID_ARG, "inv: singular")
        return o.reshape(3, 3)

    def rectify(self, im_left, im_right, rot_vec, t_vec, fill: int = 0):
        """rectify (src/automatic.cpp:66-79) -> (left_rectified, right_rectified)"""
        import torch
        im_left, im_right = _img_dev(im_left), _img_dev(im_right)
        H, W = im_left.shape[:2]
        lo, ro = torch.full_like(im_left, fill), torch.full_like(im_right, fill)
        rv = np.ascontiguousarray(rot_vec, np.float64).reshape(3)
        tv = np.ascontiguousarray(t_vec, np.float64).reshape(3)
        check(self.L.erp_rectify_dev(self.ctx.h, im_left.data_ptr(), im_right.data_ptr(), W, H,
                                     _np_ptr(rv), _np_ptr(tv), lo.data_ptr(), ro.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "rectify")
        return lo, ro

    def vertical_rotate(self, im, fill: int = 0):
        """src/automatic.cpp:148-151: rotate_image by eular2rot(RAD(89.999),0,0).inv(), then
        cv::rotate(ROTATE_90_CLOCKWISE) -> [W, H, 3]"""
        import torch
        im = _img_dev(im)
        H, W = im.shape[:2]
        out = torch.full((W, H, 3), fill, dtype=torch.uint8, device=im.device)
        check(self.L.erp_vertical_rotate_dev(self.ctx.h, im.data_ptr(), W, H, out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream),
              "vertical_rotate")
        return out

    def vertical_rotate_batch(self, ims, fill: int = 0, out=None):
        """vertical_rotate for a stack: CUDA uint8 [n, H, W, 3] -> [n, W, H, 3], byte for byte
        what n vertical_rotate calls give (erp_vertical_rotate_batch_dev: the source index of
        an output pixel is computed once for all n images).  ``out``: a caller's output stack;
        fill=-1 then leaves its unwritten pixels as they are."""
        import torch
        ims, _ = _image_batch_dev(ims, ims)
        self._on_device(ims)
        n, H, W = ims.shape[:3]
        if out is None:
            if fill < 0:
                raise ValueError("fill=-1 needs the caller's out")
            out = torch.empty((n, W, H, 3), dtype=torch.uint8, device=ims.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8
                  and out.is_contiguous() and out.shape == (n, W, H, 3)
                  and out.device == ims.device):
            raise ValueError("out is a contiguous CUDA uint8 tensor [n, W, H, 3] on ims' device")
        check(self.L.erp_vertical_rotate_batch_dev(
            self.ctx.h, ims.data_ptr() if n else None, n, W, H, int(fill),
            out.data_ptr() if n else None, torch.cuda.current_stream(ims.device).cuda_stream),
            "erp_vertical_rotate_batch_dev")
        return out

    def _on_device(self, t):
        if t.device.index != self.ctx.device:
            raise ValueError(f"images must be on the context's device cuda:{self.ctx.device}")

    def rectify_batch(self, lefts, rights, rot_vecs=None, t_vecs=None, results=None,
                      vertical: bool = True, fill: int = 0, skip=None):
        """What src/automatic.cpp:138-160 produces, for P pairs in one call: CUDA uint8
        [P, H, W, 3] left / right stacks -> {"left_rectified", "right_rectified" [P, H, W, 3],
        "done" int32 [P], and with ``vertical`` "left_vertical", "right_vertical" [P, W, H, 3]}.
        The poses are either host ``rot_vecs`` / ``t_vecs`` [P, 3] (float64, as rectify takes
        them; ``skip`` [P]: non-zero leaves a pair out) or ``results``, the device records of
        PairBatchRunner.run / run_images (uint8 [P, 64]; R, T widened to double, pairs whose
        status is not ok left out -- one readback of the records).  A pair left out or with a
        rejected pose has done = 0 and fill-valued rectified images.  Per pair the bytes are
        rectify's and vertical_rotate's."""
        import torch
        lefts, rights = _image_batch_dev(lefts, rights)
        self._on_device(lefts)
        n, H, W = lefts.shape[:3]
        if (results is None) == (rot_vecs is None and t_vecs is None) or \
                (rot_vecs is None) != (t_vecs is None):
            raise ValueError("give either rot_vecs and t_vecs or results")
        if not 0 <= int(fill) <= 255:
            raise ValueError("fill is a byte value")
        dev = lefts.device
        u8 = dict(dtype=torch.uint8, device=dev)
        out = {"left_rectified": torch.empty((n, H, W, 3), **u8),
               "right_rectified": torch.empty((n, H, W, 3), **u8),
               "done": torch.zeros(n, dtype=torch.int32, device=dev)}
        if vertical:
            out["left_vertical"] = torch.empty((n, W, H, 3), **u8)
            out["right_vertical"] = torch.empty((n, W, H, 3), **u8)
        ptr = lambda t: t.data_ptr() if n else None  # noqa: E731
        o = capi.RectifyOutputs(ptr(out["left_rectified"]), ptr(out["right_rectified"]),
                                ptr(out["left_vertical"]) if vertical else None,
                                ptr(out["right_vertical"]) if vertical else None, ptr(out["done"]))
        st = torch.cuda.current_stream(dev).cuda_stream
        if results is not None:
            if skip is not None:
                raise ValueError("skip goes with host poses; records carry their status")
            if not (isinstance(results, torch.Tensor) and results.is_cuda
                    and results.dtype == torch.uint8 and results.is_contiguous()
                    and results.shape == (n, RESULT_DTYPE.itemsize) and results.device == dev):
                raise ValueError("results is a contiguous CUDA uint8 tensor [P, 64] of "
                                 "erp_pair_result records on the images' device")
            check(self.L.erp_rectify_results_dev(self.ctx.h, ptr(lefts), ptr(rights), n, W, H,
                                                 ptr(results), int(fill), C.byref(o), st),
                  "erp_rectify_results_dev")
            return out
        rv = np.ascontiguousarray(rot_vecs, np.float64).reshape(-1, 3)
        tv = np.ascontiguousarray(t_vecs, np.float64).reshape(-1, 3)
        if rv.shape[0] != n or tv.shape[0] != n:
            raise ValueError("rot_vecs and t_vecs are [P, 3]")
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32).reshape(-1)
            if sk.shape[0] != n:
                raise ValueError("skip is [P]")
        check(self.L.erp_rectify_batch_dev(self.ctx.h, ptr(lefts), ptr(rights), n, W, H,
                                           _np_ptr(rv), _np_ptr(tv),
                                           _np_ptr(sk) if sk is not None else None, int(fill),
                                           C.byref(o), st), "erp_rectify_batch_dev")
        return out


class spherical_surf:  # noqa: N801  (reference class name)
    """spherical_surf (src/spherical_surf.hpp:11-29): the four de-distorted bands of an ERP
    image, SURF on every band, the keypoint un-rotation back to ERP pixels, the band
    concatenation, the match and the gather of the matched keypoints (do_all)."""

    PITCH = (45.0, 0.0, -45.0, -90.0)  # bands n0..n3 (src/spherical_surf.cpp:77-83)

    def __init__(self, device: int = 0, ctx: Context | None = None):
        self.ctx = ctx or Context(device)
        self.L = self.ctx.L

    def crop_rotated_image(self, pitch_rot: float, im, fill: int = 0):
        import torch
        im = _img_dev(im)
        H, W = im.shape[:2]
        out = torch.full((H // 4, W, 3), fill, dtype=torch.uint8, device=im.device)
        check(self.L.erp_crop_rotated_image_dev(self.ctx.h, im.data_ptr(), W, H, pitch_rot,
                                                out.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream),
              "crop_rotated_image")
        return out

    def bands(self, ims, fill: int = 0):
        """ims: CUDA uint8 [n, H, W, 3] (or [H, W, 3]) -> [n, 4, H/4, W, 3]"""
        import torch
        single = ims.dim() == 3
        if single:
            ims = ims.unsqueeze(0)
        if not (ims.is_cuda and ims.dtype == torch.uint8 and ims.is_contiguous()
                and ims.dim() == 4 and ims.shape[3] == 3):
            raise ValueError("images are contiguous CUDA uint8 tensors [n, H, W, 3]")
        n, H, W = ims.shape[:3]
        out = torch.full((n, 4, H // 4, W, 3), fill, dtype=torch.uint8, device=ims.device)
        check(self.L.erp_spherical_bands_dev(self.ctx.h, ims.data_ptr(), n, W, H, out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "bands")
        return out[0] if single else out

    def rotate_keypoint(self, pitch_rot_inv: float, key, width: int, height: int):
        """in place on a CUDA float32 tensor [n, 2] of (pt.x, pt.y)"""
        import torch
        check(self.L.erp_rotate_keypoints_dev(self.ctx.h, key.data_ptr(), key.shape[0],
                                              pitch_rot_inv, width, height,
                                              torch.cuda.current_stream().cuda_stream),
              "rotate_keypoint")
        return key

    def do_all(self, im_left, im_right, max_kp: int = 16384, fill: int = 0, draw: bool = False):
        """spherical_surf::do_all (src/spherical_surf.cpp:65-180) on two CUDA uint8 BGR ERP
        images [H, W, 3]: bands (:77-93) -> SURF on the 8 bands (:96-118) -> keypoint
        un-rotation + concatenation n0..n3 (:120-150) -> match_two_image (:153) -> gather
        (:155-162).  Returns (left_key [M, 2], right_key [M, 2]) CUDA float32 tensors of the
        matched ERP pixels, match_size and total_key_num (the left keypoints, :179); with
        draw=True also match_output (feature_matcher.draw_match of the two images, :173)."""
        import torch
        H, W = im_left.shape[:2]
        ims = torch.stack([_img_dev(im_left), _img_dev(im_right)]).contiguous()
        bands = self.bands(ims, fill=fill)                      # [2, 4, H/4, W, 3]
        fm = feature_matcher(ctx=self.ctx)
        kp, desc, counts = fm.surf_dev(bands.reshape(8, H // 4, W, 3), max_kp=max_kp)
        kxy = kp.view(torch.float32)[..., :2]                   # pt.x, pt.y of every row
        keys, dcat = [], []
        for side in range(2):
            c4 = [int(c) for c in counts[4 * side: 4 * side + 4]]
            key = torch.cat([kxy[4 * side + b, :c4[b]] for b in range(4)]).contiguous()
            if key.shape[0]:
                self.unrotate_band_keypoints(key, c4, W, H)
            keys.append(key)
            dcat.append(torch.cat([desc[4 * side + b, :c4[b]] for b in range(4)]).contiguous())
        m = fm._match_device(dcat[0], dcat[1], 0.3)            # [M, 4] int32 DMatch rows
        q, t = m[:, 0].long(), m[:, 1].long()
        kl, kr = keys[0][q], keys[1][t]
        if draw:
            return (kl, kr, int(m.shape[0]), int(keys[0].shape[0]),
                    fm.draw_match(im_left, im_right, kl, kr))
        return kl, kr, int(m.shape[0]), int(keys[0].shape[0])

    def pack_band_features(self, kp, desc, counts, W: int, H: int):
        """erp_pack_band_features_dev: SURF's padded output for the bands of P pairs in the
        order [pair][left, right][n0..n3] -- kp uint8 [8P, max_kp, 28], desc float32
        [8P, max_kp, 64] (feature_matcher.surf_dev's layout), counts int32 [8P] (CUDA tensor or
        host array; max_nq / max_nt come from a host copy) -- of W x H ERP images -> the dict
        do_all_batch returns."""
        import torch
        if not (isinstance(kp, torch.Tensor) and isinstance(desc, torch.Tensor) and kp.is_cuda
                and desc.is_cuda and kp.dtype == torch.uint8 and desc.dtype == torch.float32
                and kp.is_contiguous() and desc.is_contiguous() and kp.dim() == 3
                and desc.dim() == 3 and kp.shape[2] == 28 and desc.shape[2] == 64
                and kp.shape[:2] == desc.shape[:2] and kp.shape[0] % 8 == 0
                and kp.shape[1] >= 1):
            raise ValueError("kp / desc are contiguous CUDA tensors uint8 [8P, max_kp, 28] / "
                             "float32 [8P, max_kp, 64]")
        n8, max_kp = kp.shape[:2]
        if isinstance(counts, torch.Tensor):
            host = counts.detach().cpu().numpy()
        else:
            host = np.asarray(counts)
        host = np.ascontiguousarray(host, np.int32).reshape(-1)
        if host.shape[0] != n8:
            raise ValueError("counts must have one entry per band image")
        if W < 1 or H < 4:
            raise ValueError("pack_band_features needs W >= 1 and H >= 4")
        cnt = torch.from_numpy(host).to(kp.device)
        c = np.clip(host, 0, max_kp).reshape(-1, 2, 4).astype(np.int64)
        per = c.sum(axis=2)                                      # [P, 2]
        rows_l, rows_r = int(per[:, 0].sum()), int(per[:, 1].sum())
        buf = _PackedBuffers(n8 // 8, rows_l, rows_r, kp.device)
        pk = buf.struct()
        check(self.L.erp_pack_band_features_dev(self.ctx.h, kp.data_ptr(), desc.data_ptr(),
                                                cnt.data_ptr(), n8 // 8, max_kp, W, H,
                                                C.byref(pk),
                                                torch.cuda.current_stream(kp.device).cuda_stream),
              "erp_pack_band_features_dev")
        out = buf.result(rows_l, rows_r)
        out["max_nq"] = int(per[:, 0].max()) if len(per) else 0
        out["max_nt"] = int(per[:, 1].max()) if len(per) else 0
        return out

    def do_all_batch(self, lefts, rights, max_kp: int = 16384, fill: int = 0,
                     max_group_pairs: int = 0, **surf_params):
        """do_all up to the match for P pairs at once, on the device: CUDA uint8 [P, H, W, 3]
        left / right ERP batches -> bands -> SURF -> un-rotation + concatenation, as the dict
        of PairBatchRunner.run's arguments (desc_l, desc_r, kp_l, kp_r, off_l, off_r, width,
        height, max_nq, max_nt) plus band_counts [P, 2, 4].  Output buffers and max_kp grow and
        the call repeats while it reports an overflow (erp_image_pairs_features_dev);
        ``last_info`` keeps the final call's erp_image_batch_info."""
        return self._image_pairs(lefts, rights, max_kp, fill, max_group_pairs, surf_params,
                                 lambda *a: self.L.erp_image_pairs_features_dev(*a),
                                 "erp_image_pairs_features_dev")

    def _image_pairs(self, lefts, rights, max_kp, fill, max_group_pairs, surf_params, launch,
                     where):
        """the grow-and-retry loop around a library call with erp_image_pairs_features_dev's
        leading arguments (ctx .. info, stream)"""
        import torch
        lefts, rights = _image_batch_dev(lefts, rights)
        if lefts.device.index != self.ctx.device:
            raise ValueError(f"images must be on the context's device cuda:{self.ctx.device}")
        n_pairs, H, W = lefts.shape[:3]
        prm = _surf_params(self.L, surf_params)
        st = torch.cuda.current_stream(lefts.device).cuda_stream
        return self._grow_and_retry(
            n_pairs, lefts.device, max_kp, where,
            lambda kp, pk, info: launch(self.ctx.h, lefts.data_ptr(), rights.data_ptr(), n_pairs,
                                        W, H, C.byref(prm), kp, fill, max_group_pairs, pk, info,
                                        st))

    def _grow_and_retry(self, n_pairs, device, max_kp, where, call):
        """call(max_kp, byref(packed), byref(info)) -> status, repeated with a larger max_kp and
        larger output buffers while the library reports an overflow"""
        cap_l = cap_r = 1024 * max(n_pairs, 1)
        while True:
            buf = _PackedBuffers(n_pairs, cap_l, cap_r, device)
            pk = buf.struct()
            info = capi.ImageBatchInfo()
            check(call(max_kp, C.byref(pk), C.byref(info)), where)
            if info.fits:
                break
            max_kp = max(max_kp, info.need_kp)
            cap_l, cap_r = max(cap_l, info.rows_l), max(cap_r, info.rows_r)
        self.last_info = {f: getattr(info, f) for f, _ in capi.ImageBatchInfo._fields_}
        out = buf.result(info.rows_l, info.rows_r)
        out["max_nq"], out["max_nt"] = info.max_nq, info.max_nt
        return out

    def do_all_sweep(self, left, right_base, rot_mats, max_kp: int = 16384, fill: int = 0,
                     max_group_pairs: int = 0, **surf_params):
        """do_all up to the match for a rotation sweep (erp_image_sweep_features_dev): one left
        image against rotate_image(right_base, inv(rot_mat)) for every pose rot_mat of rot_mats
        (host, [P, 3, 3] float64), CUDA uint8 [H, W, 3] images -> the dict do_all_batch returns
        for the P pairs (left repeated, right images rotated), byte for byte.  The left image's
        features are computed once and the rotated images exist one group at a time."""
        return self._sweep(left, right_base, rot_mats, max_kp, fill, max_group_pairs, surf_params,
                           lambda *a: self.L.erp_image_sweep_features_dev(*a),
                           "erp_image_sweep_features_dev")

    def _sweep(self, left, right_base, rot_mats, max_kp, fill, max_group_pairs, surf_params,
               launch, where):
        """the grow-and-retry loop around a library call with erp_image_sweep_features_dev's
        leading arguments (ctx .. info, stream)"""
        import torch
        left, right_base, mats = _sweep_inputs(left, right_base, rot_mats, self.ctx.device)
        H, W = left.shape[:2]
        prm = _surf_params(self.L, surf_params)
        st = torch.cuda.current_stream(left.device).cuda_stream
        return self._grow_and_retry(
            mats.shape[0], left.device, max_kp, where,
            lambda kp, pk, info: launch(self.ctx.h, left.data_ptr(), right_base.data_ptr(),
                                        mats.shape[0], _np_ptr(mats), W, H, C.byref(prm), kp,
                                        fill, max_group_pairs, pk, info, st))

    def unrotate_band_keypoints(self, key, counts, width: int, height: int):
        """do_all's keypoint step (src/spherical_surf.cpp:120-144), in place on the band
        keypoints concatenated n0, n1, n2, n3 (CUDA float32 [n, 2]); counts = 4 band sizes"""
        import torch
        c = np.ascontiguousarray(counts, np.int32).reshape(4)
        if int(c.sum()) != key.shape[0]:
            raise ValueError("counts do not sum to the keypoint count")
        check(self.L.erp_unrotate_band_keypoints_dev(self.ctx.h, key.data_ptr(), _np_ptr(c),
                                                     width, height,
                                                     torch.cuda.current_stream().cuda_stream),
              "unrotate_band_keypoints")
        return key


def _image_batch_dev(lefts, rights):
    """the [P, H, W, 3] image batches of do_all_batch / run_images, checked before any call"""
    import torch
    for t in (lefts, rights):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8
                and t.dim() == 4 and t.shape[3] == 3 and t.is_contiguous()):
            raise ValueError("image batches are contiguous CUDA uint8 tensors [P, H, W, 3]")
    if lefts.shape != rights.shape or lefts.device != rights.device:
        raise ValueError("lefts and rights differ in shape or device")
    if lefts.shape[1] < 4 or lefts.shape[2] < 1:
        raise ValueError("images need H >= 4 and W >= 1")
    return lefts, rights


_stereo_ctx: dict = {}


class stereo:  # noqa: N801  (a namespace, as the reference-named classes above)
    """Dense disparity on row-rectified views (include/erp_match.h "dense stereo on
    row-rectified views"): census + 4- or 8-path SGM, sub-pixel winner, left-right check, optional
    depth.  Images are contiguous CUDA uint8 tensors [rows, cols] (gray), [rows, cols, C] or
    [P, rows, cols, C] with C = 1 or 3 (BGR); the outputs have the images' shape without C."""

    @staticmethod
    def disparity(left, right, *, d_min: int = 0, n_disp: int = 64, p1: int = 8, p2: int = 64,
                  lr_max: int = 1, wrap_rows: int = 0, n_paths: int = 4, uniqueness: int = 0,
                  depth: bool = False, ctx=None):
        """erp_stereo_rows_dev -> disp16 (int16, the left image's disparity in 1/16 pixel,
        capi.STEREO_INVALID where rejected), or (disp16, depth float32) with ``depth``.
        ``n_paths`` = 8 adds the four diagonal paths (rule 4b), ``uniqueness`` = 1..99 the
        uniqueness test in percent (rule 6b); either goes through erp_stereo_rows_ex_dev, the
        defaults through the call above.
        Asynchronous on torch's current stream.  ctx=None: one context per device, kept."""
        import torch
        for t in (left, right):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8
                    and t.is_contiguous() and 2 <= t.dim() <= 4
                    and (t.dim() == 2 or t.shape[-1] in (1, 3))):
                raise ValueError("views are contiguous CUDA uint8 tensors [rows, cols], "
                                 "[rows, cols, C] or [P, rows, cols, C], C = 1 or 3")
        if left.shape != right.shape or left.device != right.device:
            raise ValueError("left and right differ in shape or device")
        dev = left.device
        if ctx is None:
            ctx = _stereo_ctx.get(dev.index)
            if ctx is None:
                ctx = _stereo_ctx[dev.index] = Context(dev.index)
        elif dev.index != ctx.device:
            raise ValueError(f"views must be on the context's device cuda:{ctx.device}")
        shape = tuple(left.shape) if left.dim() == 2 else tuple(left.shape[:-1])
        n = shape[0] if left.dim() == 4 else 1
        rows, cols = shape[-2:]
        par = capi.StereoParams(int(d_min), int(n_disp), int(p1), int(p2), int(lr_max),
                                int(wrap_rows), 1 if left.dim() == 2 else left.shape[-1])
        disp16 = torch.empty(shape, dtype=torch.int16, device=dev)
        z = torch.empty(shape, dtype=torch.float32, device=dev) if depth else None
        ptr = lambda t: t.data_ptr() if t is not None and n else None  # noqa: E731
        call, name = ctx.L.erp_stereo_rows_dev, "erp_stereo_rows_dev"
        if (int(n_paths), int(uniqueness)) != (4, 0):
            par = capi.StereoParamsEx(par, int(n_paths), int(uniqueness))
            call, name = ctx.L.erp_stereo_rows_ex_dev, "erp_stereo_rows_ex_dev"
        check(call(ctx.h, ptr(left), ptr(right), n, rows, cols, C.byref(par), ptr(disp16), ptr(z),
                   torch.cuda.current_stream(dev).cuda_stream), name)
        return (disp16, z) if depth else disp16

    @staticmethod
    def vertical(left_vertical, right_vertical, **kw):
        """disparity on the vertical views of erp_rotation.rectify_batch /
        PairBatchRunner.rectify_images ([P, W, H, 3]: W rows of H columns, the row index being
        longitude): wrap_rows = 1.  The keywords are disparity's; with ``n_paths`` = 8 the
        diagonal paths wrap their rows too, so every diagonal runs from pole to pole, and
        ``uniqueness`` rejects the pixels whose best sum is not that much below the others."""
        if "wrap_rows" in kw:
            raise ValueError("vertical views wrap their rows; use disparity for wrap_rows = 0")
        return stereo.disparity(left_vertical, right_vertical, wrap_rows=1, **kw)


def _rot_mats_host(rot_mats) -> np.ndarray:
    """poses as a contiguous host float64 array [P, 3, 3]"""
    try:
        import torch
        if isinstance(rot_mats, torch.Tensor):
            rot_mats = rot_mats.detach().cpu().numpy()
    except ImportError:  # pragma: no cover
        pass
    m = np.ascontiguousarray(rot_mats, np.float64)
    if not (m.shape[-2:] == (3, 3) and m.ndim in (2, 3)) and not (m.ndim == 2 and m.shape[1] == 9):
        raise ValueError("rot_mats are 3x3 matrices [P, 3, 3]")
    return m.reshape(-1, 3, 3)


def _sweep_inputs(left, right_base, rot_mats, device: int):
    """the images and poses of do_all_sweep / run_sweep, checked before any call"""
    left, right_base = _img_dev(left), _img_dev(right_base)
    if left.shape != right_base.shape or left.device != right_base.device:
        raise ValueError("left and right_base differ in shape or device")
    if left.device.index != device:
        raise ValueError(f"images must be on the context's device cuda:{device}")
    if left.shape[0] < 4 or left.shape[1] < 1:
        raise ValueError("images need H >= 4 and W >= 1")
    return left, right_base, _rot_mats_host(rot_mats)


def sweep_relative_rotation(results, initial_rot_mat) -> np.ndarray:
    """two_real_image_test/main.cpp:215-219 for a sweep's records, host only:
    result_rot_vec = rot2eular(eular2rot((double)R) * initial_rot_mat.inv()) per pose ->
    [P, 3] float64 (radians).  results: run_sweep's ``results`` (tensor or RESULT_DTYPE array)
    or the R vectors [P, 3]."""
    L = capi.load()
    try:
        import torch
        if isinstance(results, torch.Tensor):
            results = (results_to_numpy(results) if results.dtype == torch.uint8
                       else results.detach().cpu().numpy())
    except ImportError:  # pragma: no cover
        pass
    r = np.asarray(results)
    if r.dtype.names:
        r = r["R"]
    r = np.ascontiguousarray(r, np.float32).reshape(-1, 3).astype(np.float64)  # Vec3f -> Vec3d
    init = _m9(initial_rot_mat)
    inv = np.zeros(9, np.float64)
    if not L.erp_inv3(_np_ptr(init), _np_ptr(inv)):
        raise ErpError(capi.ERP_INVALID_ARG, "sweep_relative_rotation: singular initial_rot_mat")
    b = inv.reshape(3, 3)
    out = np.zeros((r.shape[0], 3), np.float64)
    a, prod = np.zeros(9, np.float64), np.zeros(9, np.float64)
    for p in range(r.shape[0]):
        L.erp_eular2rot(_np_ptr(np.ascontiguousarray(r[p])), _np_ptr(a))
        m = a.reshape(3, 3)
        for i in range(3):      # cv::gemm on 3x3 doubles: (a0 b0 + a1 b1) + a2 b2
            for j in range(3):
                prod[i * 3 + j] = (m[i, 0] * b[0, j] + m[i, 1] * b[1, j]) + m[i, 2] * b[2, j]
        L.erp_rot2eular(_np_ptr(prod), _np_ptr(out[p]))
    return out


def _surf_params(L, params):
    prm = capi.SurfParams()
    L.erp_surf_params_default(C.byref(prm))
    for k, v in params.items():
        if k not in dict(capi.SurfParams._fields_):
            raise ValueError(f"unknown SURF parameter {k!r}")
        setattr(prm, k, v)
    return prm


class _PackedBuffers:
    """caller-owned outputs of the pack step (erp_packed_pairs) as torch tensors"""

    def __init__(self, n_pairs: int, cap_l: int, cap_r: int, device):
        import torch
        f32, i64, i32 = torch.float32, torch.int64, torch.int32
        self.cap = (cap_l, cap_r)
        self.t = {"desc_l": torch.empty((max(cap_l, 1), 64), dtype=f32, device=device),
                  "desc_r": torch.empty((max(cap_r, 1), 64), dtype=f32, device=device),
                  "kp_l": torch.empty((max(cap_l, 1), 2), dtype=f32, device=device),
                  "kp_r": torch.empty((max(cap_r, 1), 2), dtype=f32, device=device),
                  "off_l": torch.zeros(n_pairs + 1, dtype=i64, device=device),
                  "off_r": torch.zeros(n_pairs + 1, dtype=i64, device=device),
                  "width": torch.zeros(max(n_pairs, 1), dtype=i32, device=device),
                  "height": torch.zeros(max(n_pairs, 1), dtype=i32, device=device),
                  "band_counts": torch.zeros((max(n_pairs, 1), 2, 4), dtype=i32, device=device)}
        self.n_pairs = n_pairs

    def struct(self) -> "capi.PackedPairs":
        t = self.t
        return capi.PackedPairs(*[t[k].data_ptr() for k in
                                  ("desc_l", "desc_r", "kp_l", "kp_r", "off_l", "off_r", "width",
                                   "height", "band_counts")], self.cap[0], self.cap[1])

    def result(self, rows_l: int, rows_r: int) -> dict:
        t, n = self.t, self.n_pairs
        return {"desc_l": t["desc_l"][:rows_l], "desc_r": t["desc_r"][:rows_r],
                "kp_l": t["kp_l"][:rows_l], "kp_r": t["kp_r"][:rows_r], "off_l": t["off_l"],
                "off_r": t["off_r"], "width": t["width"][:n], "height": t["height"][:n],
                "band_counts": t["band_counts"][:n]}


# where a record kind keeps its solved 9-vector and its status: (byte offset of E, of status)
RECORD_SOURCES = {"winners": tuple(WINNER_DTYPE.fields[k][1] for k in ("E", "status")),
                  "polish": tuple(POLISH_DTYPE.fields[k][1] for k in ("E", "status"))}


def _record_source(where: str, source: str, out: dict, polish):
    """-> (records, E offset, status offset) of select_pose's / guided_match's ``source=``: the
    winner records of run()'s dict or the polish records of polish()'s"""
    if source not in RECORD_SOURCES:
        raise ValueError(f"{where}: source is 'winners' or 'polish'")
    if source == "winners":
        if "winners" not in out:
            raise ValueError(f"{where}(source='winners') needs run(..., want=('winners',))")
        return (out["winners"], *RECORD_SOURCES[source])
    if polish is None or "polish" not in polish:
        raise ValueError(f"{where}(source='polish') needs polish=polish(...)")
    return (polish["polish"], *RECORD_SOURCES[source])


class PairBatchRunner:
    """The fused hot path over a batch of ERP pairs held in device memory (torch tensors).

    run(...) launches match -> gather -> find for every pair on torch's current stream and
    returns a torch uint8 tensor of erp_pair_result records (view with RESULT_DTYPE after
    .cpu()).  Optional debug outputs (matches, hyps, samples, rvec, tvec, dist) are allocated
    when requested; want=("winners",) adds the winner records (uint8 [P, 88], WINNER_DTYPE: the
    winning iteration's E without the hypothesis records) through erp_pair_batch_run_winners;
    want=("support",) with support_thr= adds the support stage (erp_pair_batch_run_support): the
    scored iteration most matches agree with under |l^T E' r| < support_thr, as "support" (uint8
    [P, 32], SUPPORT_DTYPE), "support_winners" (uint8 [P, 88]), "support_results" (uint8 [P, 64])
    and, with want "support_counts", every iteration's count (int32 [P, iters]).
    """

    def __init__(self, device: int = 0, ctx: Context | None = None, reuse_outputs: bool = False,
                 stream: RandStream | None = None, **cfg):
        """stream: a RandStream (not a HIP stream) the runs draw from and advance, pair after
        pair as the reference's drivers do on the process-global rand(); None: every pair of
        every run starts at cfg.seed / cfg.offset.
        reuse_outputs: run() hands back the SAME output tensors for the same shape (copy them
        before the next call) -- what a HIP-graph replay (Context.set_graphs) needs, since the
        captured graph bakes the output pointers in"""
        self.ctx = ctx or Context(device)
        self.cfg = default_cfg(**cfg)
        self.device = self.ctx.device
        self.reuse_outputs = reuse_outputs
        self._outs = {}
        if stream is not None:
            self.ctx.set_rand_stream(stream)

    def reserve(self, n_pairs: int, max_nq: int, max_nt: int):
        check(self.ctx.L.erp_ctx_reserve(self.ctx.h, n_pairs, max_nq, max_nt, self.cfg.iters),
              "erp_ctx_reserve")

    def run(self, desc_l, desc_r, kp_l, kp_r, off_l, off_r, width, height, max_nq: int,
            max_nt: int, ratio: float = 0.3, want=(), stream=None, support_thr=None):
        import torch
        want = tuple(want)
        if "support_counts" in want and "support" not in want:
            raise ValueError("want 'support_counts' needs 'support'")
        if "support" in want and "winners" in want:
            raise ValueError("want 'support' or 'winners', not both: one stage per run "
                             "(out['support_winners'] holds the support stage's winner records)")
        if "support" in want:
            support_thr = _support_thr(support_thr)
        elif support_thr is not None:
            raise ValueError("support_thr needs want=('support', ...)")
        n_pairs = off_l.shape[0] - 1
        dev = desc_l.device
        for t, dt in ((desc_l, torch.float32), (desc_r, torch.float32), (kp_l, torch.float32),
                      (kp_r, torch.float32), (off_l, torch.int64), (off_r, torch.int64),
                      (width, torch.int32), (height, torch.int32)):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                raise ValueError("batch tensors must be contiguous CUDA tensors of the C types")
        b = capi.PairBatch(n_pairs, desc_l.shape[1], max_nq, max_nt, desc_l.data_ptr(),
                           desc_r.data_ptr(), kp_l.data_ptr(), kp_r.data_ptr(), off_l.data_ptr(),
                           off_r.data_ptr(), width.data_ptr(), height.data_ptr())
        key = (n_pairs, max_nq, tuple(want), str(dev), self.cfg.iters)
        if self.reuse_outputs and key in self._outs:
            outs = self._outs[key]
            return self._launch(b, ratio, outs, stream, dev, support_thr)
        outs = {"results": torch.empty((n_pairs, RESULT_DTYPE.itemsize), dtype=torch.uint8,
                                       device=dev)}
        iters = self.cfg.iters
        s_max = max(int(max_nq * self.cfg.sample_frac), 1)
        shapes = {"matches": (n_pairs, max_nq, 4, torch.int32),
                  "key_left": (n_pairs, max_nq, 2, torch.float32),
                  "key_right": (n_pairs, max_nq, 2, torch.float32),
                  "hyps": (n_pairs, iters, HYP_DTYPE.itemsize, torch.uint8),
                  "samples": (n_pairs, iters, s_max, torch.int32),
                  "rvec": (n_pairs, 2 * iters, 3, torch.float32),
                  "tvec": (n_pairs, 2 * iters, 3, torch.float32),
                  "dist": (n_pairs, 2 * iters, torch.float64),
                  "winners": (n_pairs, WINNER_DTYPE.itemsize, torch.uint8),
                  "support": (n_pairs, SUPPORT_DTYPE.itemsize, torch.uint8),
                  "support_counts": (n_pairs, iters, torch.int32)}
        if "support" in want:
            outs["support_winners"] = torch.zeros((n_pairs, WINNER_DTYPE.itemsize),
                                                  dtype=torch.uint8, device=dev)
            outs["support_results"] = torch.zeros((n_pairs, RESULT_DTYPE.itemsize),
                                                  dtype=torch.uint8, device=dev)
        for name in want:
            *shape, dt = shapes[name]
            outs[name] = torch.zeros(shape, dtype=dt, device=dev)
        if self.reuse_outputs:
            self._outs[key] = outs
        return self._launch(b, ratio, outs, stream, dev, support_thr)

    @staticmethod
    def support_view(out: dict) -> dict:
        """run(..., want=("support", ...))'s dict with the support stage's records in the
        consensus winner's place: {**out, "results": support_results, "winners":
        support_winners}, which polish(), select_pose() and guided_match() take unchanged."""
        if "support_results" not in out or "support_winners" not in out:
            raise ValueError("support_view needs run(..., want=('support', ...))")
        return {**out, "results": out["support_results"], "winners": out["support_winners"]}

    def run_images(self, lefts, rights, ratio: float = 0.3, want=(), max_kp: int = 16384,
                   fill: int = 0, max_group_pairs: int = 0, **surf_params):
        """run() from the ERP images: CUDA uint8 [P, H, W, 3] left / right batches ->
        spherical_surf.do_all_batch's packed batch -> match -> gather -> find -> the same
        ``outs`` dict as run().  Without optional outputs this is one library call
        (erp_image_pairs_run); with them (their shapes depend on the packed batch's max_nq) it
        is do_all_batch followed by run().  ``last_packed`` keeps the packed batch.  Not
        graph-capturable (the feature stage synchronises per group of pairs)."""
        import torch
        lefts, rights = _image_batch_dev(lefts, rights)
        n_pairs = lefts.shape[0]
        ss = spherical_surf(ctx=self.ctx)
        if want and n_pairs:
            p = ss.do_all_batch(lefts, rights, max_kp=max_kp, fill=fill,
                                max_group_pairs=max_group_pairs, **surf_params)
            self.last_packed, self.last_info = p, ss.last_info
            return self.run(*[p[k] for k in ("desc_l", "desc_r", "kp_l", "kp_r", "off_l", "off_r",
                                             "width", "height", "max_nq", "max_nt")],
                            ratio=ratio, want=want)
        res = torch.empty((max(n_pairs, 1), RESULT_DTYPE.itemsize), dtype=torch.uint8,
                          device=lefts.device)

        def launch(h, l_ptr, r_ptr, n, W, H, prm, kp, fl, grp, pk, info, st):
            o = capi.BatchOutputs(res.data_ptr())
            return self.ctx.L.erp_image_pairs_run(h, l_ptr, r_ptr, n, W, H, prm, kp, fl, grp, pk,
                                                  ratio, C.byref(self.cfg), C.byref(o), info, st)
        self.last_packed = ss._image_pairs(lefts, rights, max_kp, fill, max_group_pairs,
                                           surf_params, launch, "erp_image_pairs_run")
        self.last_info = ss.last_info
        return {"results": res[:n_pairs]}

    def rectify_images(self, lefts, rights, ratio: float = 0.3, vertical: bool = True,
                       rect_fill: int = 0, **run_images_kwargs):
        """automatic's main (src/automatic.cpp:81-164) for a batch: run_images, then
        erp_rotation.rectify_batch on its device records -> run_images' dict plus
        left_rectified, right_rectified, done and (``vertical``) left_vertical, right_vertical.
        A pair whose status is not ok has done = 0 and rect_fill-valued rectified images."""
        outs = dict(self.run_images(lefts, rights, ratio=ratio, **run_images_kwargs))
        outs.update(erp_rotation(ctx=self.ctx).rectify_batch(
            lefts, rights, results=outs["results"].contiguous(), vertical=vertical,
            fill=rect_fill))
        return outs

    def run_sweep(self, left, right_base, rot_mats, ratio: float = 0.3, want=(),
                  match_error: bool = True, chunk: int = 128, max_kp: int = 16384, fill: int = 0,
                  max_group_pairs: int = 0, **surf_params):
        """The reference drivers' rotation sweep (one_image_test/main.cpp:73-145 and the two
        16^3 drivers): one left image against rotate_image(right_base, inv(rot_mat)) for every
        pose of rot_mats (host [P, 3, 3]) -> {"results": records [P], "match_error": CUDA
        float64 [P] (the drivers' "Surf match error", radians; match_error=False leaves it
        out), ...}.  The left image's features are computed once per library call and the poses
        go through in chunks of ``chunk`` per call (erp_image_sweep_run), so the rotated images
        and the packed buffers stay bounded whatever P; with a RandStream attached the poses
        draw from it one after the other.  Optional outputs (``want``, as run()) need
        P <= chunk -- their shapes depend on the chunk's max_nq -- and take the route
        do_all_sweep -> run() -> erp_rotation.match_error.  ``last_packed`` / ``last_info``
        keep the last chunk's packed batch and info."""
        import torch
        left, right_base, mats = _sweep_inputs(left, right_base, rot_mats, self.ctx.device)
        n, chunk = mats.shape[0], int(chunk)
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        if want and n > chunk:
            raise ValueError("optional outputs need every pose in one chunk (P <= chunk)")
        H, W = left.shape[:2]
        dev = left.device
        ss = spherical_surf(ctx=self.ctx)
        if want and n:
            p = ss.do_all_sweep(left, right_base, mats, max_kp=max_kp, fill=fill,
                                max_group_pairs=max_group_pairs, **surf_params)
            self.last_packed, self.last_info = p, ss.last_info
            keys = ("key_left", "key_right") if match_error else ()
            outs = self.run(*[p[k] for k in ("desc_l", "desc_r", "kp_l", "kp_r", "off_l", "off_r",
                                             "width", "height", "max_nq", "max_nt")],
                            ratio=ratio, want=tuple(want) + tuple(k for k in keys if k not in want))
            res = {k: v for k, v in outs.items() if k == "results" or k in want}
            if match_error:
                m_col = outs["results"].view(torch.int32)[:, RESULT_DTYPE.fields["M"][1] // 4]
                res["match_error"] = erp_rotation(ctx=self.ctx).match_error(
                    outs["key_left"], outs["key_right"], m_col, mats, W, H)
            return res
        res = torch.empty((max(n, 1), RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        err = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        for c0 in range(0, n, chunk):
            c1 = min(n, c0 + chunk)

            def launch(h, l_ptr, r_ptr, n_poses, m_ptr, W_, H_, prm, kp, fl, grp, pk, info, st):
                o = capi.BatchOutputs(res[c0:].data_ptr())
                return self.ctx.L.erp_image_sweep_run(
                    h, l_ptr, r_ptr, n_poses, m_ptr, W_, H_, prm, kp, fl, grp, pk, ratio,
                    C.byref(self.cfg), C.byref(o), err[c0:].data_ptr() if match_error else None,
                    info, st)
            self.last_packed = ss._sweep(left, right_base, mats[c0:c1], max_kp, fill,
                                         max_group_pairs, surf_params, launch,
                                         "erp_image_sweep_run")
            self.last_info = ss.last_info
            max_kp = max(max_kp, self.last_info["need_kp"])  # the next chunk starts where this fit
        out = {"results": res[:n]}
        if match_error:
            out["match_error"] = err[:n]
        return out

    def polish(self, out: dict, width, height, thr: float, rounds: int = 3,
               want_rounds: bool = False, stream=None) -> dict:
        """The polish stage (include/erp_match.h "polish"; no reference counterpart) on the dict
        ``run(..., want=("hyps", "key_left", "key_right"))`` returned -- or, without the
        hypothesis records, ``want=("winners", "key_left", "key_right")`` (the lite route;
        ``hyps`` is used when both are there): the inlier set of every
        pair's winner under |l^T E' r| < thr and up to ``rounds`` refits on it -> {"polish":
        records (polish_to_numpy), "mask": uint8 [P, max_nq] (1 = inlier of the final state),
        "rounds": the per-round records (want_rounds; polish_rounds_to_numpy)}.  One launch on
        torch's current stream (or ``stream``), nothing leaves the device; ``out`` is only read."""
        missing = [k for k in ("results", "key_left", "key_right") if k not in out]
        if "hyps" not in out and "winners" not in out:
            missing.append("hyps")
        if missing:
            raise ValueError(f"polish needs run(..., want=('hyps', 'key_left', 'key_right')) or "
                             f"want=('winners', 'key_left', 'key_right'): missing {missing}")
        use_hyps = "hyps" in out
        return self.ctx.polish(out["results"], out["hyps"] if use_hyps else None, out["key_left"],
                               out["key_right"], width, height, thr, rounds=rounds,
                               valid_abs=self.cfg.valid_abs, want_rounds=want_rounds,
                               stream=stream, winners=None if use_hyps else out["winners"])

    def select_pose(self, out: dict, width, height, source: str = "winners", polish: dict | None = None,
                    thr: float = 0.0, min_sin2: float = 0.0,
                    want=("depth", "front", "results"), stream=None) -> dict:
        """The pose selection (include/erp_match.h "pose selection"; no reference counterpart) on
        the dict ``run(..., want=("winners", "key_left", "key_right"))`` returned: the cheirality
        vote over (R1 | R2) x (+t | -t) per pair.  source="winners": on the winners' E, every
        match with |l^T E' r| < thr voting (thr <= 0: every match); source="polish": on the E
        and the inlier mask of ``polish`` (what polish() returned; thr is normally 0 then).
        -> {"pose": records (pose_to_numpy), "depth": float64 [P, max_nq, 2], "front": uint8
        [P, max_nq], "results": the result records with the selected R, T (they feed
        rectify_batch(results=...))}.  One launch on torch's current stream (or ``stream``);
        ``out`` and ``polish`` are only read."""
        need = ["results", "key_left", "key_right"] + (["winners"] if source == "winners" else [])
        missing = [k for k in need if k not in out]
        if missing:
            raise ValueError(f"select_pose needs run(..., want=('winners', 'key_left', "
                             f"'key_right')): missing {missing}")
        if source == "polish" and (polish is None or "polish" not in polish or "mask" not in polish):
            raise ValueError("select_pose(source='polish') needs polish=polish(...) with its mask")
        src, e_off, s_off = _record_source("select_pose", source, out, polish)
        mask = polish["mask"] if source == "polish" else None
        return self.ctx.select_pose(out["results"], out["key_left"], out["key_right"], width,
                                    height, src, e_off, s_off, mask=mask, thr=thr,
                                    min_sin2=min_sin2, want=want, stream=stream)

    def guided_match(self, out: dict, desc_l, desc_r, kp_l, kp_r, off_l, off_r, width, height,
                     max_nq: int, max_nt: int | None = None, *, source: str = "winners",
                     polish: dict | None = None, thr: float, ratio: float = 0.8,
                     max_dist: float = 0.0, unique: bool = True,
                     want=("matches", "key_left", "key_right", "gated", "results", "winners"),
                     stream=None) -> dict:
        """Guided matching (include/erp_match.h "guided matching"; no reference counterpart)
        behind ``run(..., want=("winners", ...))`` on the same packed batch: every pair's
        descriptors rematched inside the epipolar band |l^T E' r| < thr of its solved E, with
        the ratio test d0 < ratio * d1 inside the band.  source="winners": the E of out["winners"];
        source="polish": the E of ``polish`` (what polish() returned).  -> {"results", "winners",
        "key_left", "key_right", "matches", "count", "gated"} (``want`` names all but count):
        results = out's records with M replaced by the guided count and winners = records that
        carry E, so polish() and select_pose() take the returned dict as they take run()'s.  Three
        launches on torch's current stream (or ``stream``); ``out`` and ``polish`` are only read.
        max_nt=None reads the largest right row count from off_r (a device-to-host copy)."""
        if max_nt is None:
            max_nt = int((off_r[1:] - off_r[:-1]).max().item()) if off_r.numel() > 1 else 0
        if "results" not in out:
            raise ValueError("guided_match needs run()'s dict with its results")
        src, e_off, s_off = _record_source("guided_match", source, out, polish)
        return self.ctx.guided_match(desc_l, desc_r, kp_l, kp_r, off_l, off_r, width, height,
                                     max_nq, max_nt, src, e_off, s_off, results=out["results"],
                                     thr=thr, ratio=ratio, max_dist=max_dist, unique=unique,
                                     want=want, stream=stream)

    def _launch(self, b, ratio, outs, stream, dev, support_thr=None):
        import torch
        o = capi.BatchOutputs(*[outs[k].data_ptr() if k in outs else None
                                for k in ("results", "matches", "key_left", "key_right", "hyps",
                                          "samples", "rvec", "tvec", "dist")])
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        if "winners" in outs:
            check(self.ctx.L.erp_pair_batch_run_winners(self.ctx.h, C.byref(b), ratio,
                                                        C.byref(self.cfg), C.byref(o),
                                                        outs["winners"].data_ptr(), st),
                  "erp_pair_batch_run_winners")
            return outs
        if "support" in outs:
            so = capi.SupportOutputs(outs["support"].data_ptr(), outs["support_winners"].data_ptr(),
                                     outs["support_results"].data_ptr(),
                                     outs["support_counts"].data_ptr()
                                     if "support_counts" in outs else None)
            check(self.ctx.L.erp_pair_batch_run_support(self.ctx.h, C.byref(b), ratio,
                                                        C.byref(self.cfg), C.byref(o), support_thr,
                                                        C.byref(so), st),
                  "erp_pair_batch_run_support")
            return outs
        check(self.ctx.L.erp_pair_batch_run(self.ctx.h, C.byref(b), ratio, C.byref(self.cfg),
                                            C.byref(o), st), "erp_pair_batch_run")
        return outs


def results_to_numpy(t) -> np.ndarray:
    return t.cpu().numpy().view(RESULT_DTYPE).reshape(-1)


def polish_to_numpy(t) -> np.ndarray:
    """erp_polish_result records (Context.polish / PairBatchRunner.polish "polish") -> [P]"""
    return t.cpu().numpy().view(POLISH_DTYPE).reshape(-1)


def winners_to_numpy(t) -> np.ndarray:
    """erp_winner records (run(..., want=("winners",)) "winners") -> [P]"""
    return t.cpu().numpy().view(WINNER_DTYPE).reshape(-1)


def pose_to_numpy(t) -> np.ndarray:
    """erp_pose records (Context.select_pose / PairBatchRunner.select_pose "pose") -> [P]"""
    return t.cpu().numpy().view(POSE_DTYPE).reshape(-1)


def polish_rounds_to_numpy(t) -> np.ndarray:
    """erp_polish_round records ("rounds") -> [P, rounds]"""
    a = t.cpu().numpy()
    return a.reshape(a.shape[0], -1).view(POLISH_ROUND_DTYPE)


def hyps_to_numpy(t) -> np.ndarray:
    a = t.cpu().numpy()
    return a.reshape(a.shape[0], -1).view(HYP_DTYPE)
