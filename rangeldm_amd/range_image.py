"""Range image <-> point cloud on the GPU: the host-side mirror of the reference's `point_cloud_to_range_image`
(ldm/dataset.py:135-294) and its sensor subclasses (ldm/kitti360_range_image.py:14-61,
ldm/nuscenes_range_image.py:16-46).  Same class / method / argument names; every method hands device tensors to
librangeldm_hip.so (rangeldm_amd/csrc/lidar.hip) and returns freshly allocated device tensors.  No CPU fallback.

Differences a caller can observe (both deliberate):
  * `to_pc_torch` does not need a mutable input (the reference rewrites `r_true` in a temporary, too);
  * `__call__` does not shift the caller's `pc[:, 2]` in place (ldm/dataset.py:168 does).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


class point_cloud_to_range_image:
    def __init__(self, width=1024, grid_sizes=[1, 1024, 1024], pc_range=[-25.6, -25.6, -3., 25.6, 25.6, 1.], log=False,
                 normalize_volume_densities=True, inverse=False) -> None:
        self.range_fill_value = np.array([100, 0])
        self.width = width
        self.grid_sizes = list(grid_sizes)
        self.pc_range = list(pc_range)
        self.log = log
        self.normalize_volume_densities = normalize_volume_densities
        self.inverse = inverse
        self.mean = 20.
        self.std = 40.
        self.min_depth = 0.0            # nuScenes drops returns closer than 2 m before projecting
        if not hasattr(self, "incl"):
            self.height = self.zenith = self.incl = None
            self.H = None
        self._h = None

    # ---- handle ---------------------------------------------------------------------------------------------
    def _handle(self):
        if self._h is None:
            if self.incl is None:
                raise NotImplementedError("sensor tables (incl / height) are defined by the subclasses")
            _lib.require_gpu()
            cfg = _lib.LidarConfigC()
            cfg.beams, cfg.width = int(self.H), int(self.width)
            cfg.mode = 1 if self.log else (2 if self.inverse else 0)
            cfg.mean, cfg.std = float(self.mean), float(self.std)
            cfg.range_fill, cfg.intensity_fill = float(self.range_fill_value[0]), float(self.range_fill_value[1])
            for i in range(3):
                cfg.grid[i] = int(self.grid_sizes[i])
            for i in range(6):
                cfg.pc_range[i] = float(self.pc_range[i])
            cfg.normalize_volume_densities = int(bool(self.normalize_volume_densities))
            incl = np.ascontiguousarray(self.incl, np.float32)
            height = np.ascontiguousarray(self.height, np.float32)
            h = C.c_void_p()
            _lib.check(_lib.lib().rldm_lidar_create(C.byref(cfg), incl.ctypes.data_as(C.POINTER(C.c_float)),
                                                    height.ctypes.data_as(C.POINTER(C.c_float)), C.byref(h)),
                       "rldm_lidar_create")
            self._h = h
        return self._h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            try:
                _lib.lib().rldm_lidar_destroy(h)
            except Exception:
                pass

    def _images(self, range_images):
        if range_images.dim() != 4 or range_images.shape[3] != self.H:
            raise ValueError(f"range_images must be (B, C, W, {self.H}), got {tuple(range_images.shape)}")
        if not range_images.is_cuda:
            raise RuntimeError("range_images must live on the GPU (rangeldm_amd has no CPU path)")
        return range_images.detach().float().contiguous()

    # ---- f1: after the sampler ------------------------------------------------------------------------------
    def to_pc_torch(self, range_images):
        """range_images: B x C x W x H -> point_cloud: B x N x (4 if C > 1 else 3)   (ldm/dataset.py:228-278)"""
        x = self._images(range_images)
        B, Cc, W, H = x.shape
        out = torch.empty((B, W * H, 4 if Cc > 1 else 3), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().rldm_lidar_to_points(self._handle(), x.data_ptr(), B, Cc, W, out.data_ptr(),
                                                   _lib.stream_ptr(x.device)), "rldm_lidar_to_points")
        return out

    def to_voxel(self, range_images, ordered=False):
        """-> (B, 2 * D, H, W) BEV volume: vote density and density-normalised remission (ldm/dataset.py:280-294).  ordered: the
        order-fixed splat of to_voxel_train(ordered=True) -- the same bits on every run, slower."""
        if ordered:
            return self.to_voxel_train(range_images, ordered=True)[0]
        x = self._images(range_images)
        B, Cc, W, H = x.shape
        D, GH, GW = self.grid_sizes
        out = torch.empty((B, 2 * D, GH, GW), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().rldm_lidar_to_voxel(self._handle(), x.data_ptr(), B, Cc, W, out.data_ptr(),
                                                  _lib.stream_ptr(x.device)), "rldm_lidar_to_voxel")
        return out

    # ---- to_voxel for training (vae_training.py: disc_bev, bev_rec_weight) ----------------------------------
    def to_voxel_train(self, range_images, ordered=False):
        """`to_voxel` that keeps what its backward needs: -> (voxel, saved).  voxel holds the bits `to_voxel` returns; saved =
        (the fp32 image, raw (B, 2 * D, H, W): the vote density d and the weighted remission sum S before the finalise step).
        ordered: rldm_lidar_to_voxel_ordered instead of the atomic splat -- every cell the fp32 sum of its votes in ascending vote
        id (to_voxel_ordered_host states it), so the result is the same on every run, for every batch size and batch position."""
        x = self._images(range_images)
        B, Cc, W, H = x.shape
        D, GH, GW = self.grid_sizes
        raw = torch.empty((B, 2 * D, GH, GW), dtype=torch.float32, device=x.device)
        out = torch.empty_like(raw)
        if ordered:
            _lib.check(_lib.lib().rldm_lidar_to_voxel_ordered(self._handle(), x.data_ptr(), B, Cc, W, raw.data_ptr(), out.data_ptr(),
                                                              _lib.stream_ptr(x.device)), "rldm_lidar_to_voxel_ordered")
        else:
            _lib.check(_lib.lib().rldm_lidar_to_voxel_train(self._handle(), x.data_ptr(), B, Cc, W, raw.data_ptr(), out.data_ptr(),
                                                            _lib.stream_ptr(x.device)), "rldm_lidar_to_voxel_train")
        return out, (x, raw)

    def to_voxel_backward(self, saved, dvoxel):
        """d(loss) / d(range_images) (B, 2, W, H) for d(loss) / d(voxel) = dvoxel (B, 2 * D, H, W) and `saved` of to_voxel_train: two
        launches, no atomics, bit-reproducible (rldm_lidar_to_voxel_backward).  Channels beyond the first two get no vote and no
        gradient."""
        x, raw = saved
        B, Cc, W, H = x.shape
        if tuple(dvoxel.shape) != tuple(raw.shape) or not dvoxel.is_cuda:
            raise ValueError(f"dvoxel must be a device tensor of shape {tuple(raw.shape)}, got {tuple(dvoxel.shape)}")
        g = dvoxel.detach().float().contiguous()
        cell = torch.empty_like(raw)
        out = torch.empty((B, 2, W, H), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().rldm_lidar_to_voxel_backward(self._handle(), x.data_ptr(), B, Cc, W, raw.data_ptr(), g.data_ptr(),
                                                           cell.data_ptr(), out.data_ptr(), _lib.stream_ptr(x.device)),
                   "rldm_lidar_to_voxel_backward")
        return out

    # ---- host statements of to_voxel and its backward (plain torch; the tests' references) -------------------
    def _bev_geometry(self, x, points=None, tables="reference"):
        """What bev_splat_kernel computes per pixel before it votes, in x's dtype, one torch operation per device operation (in fp32
        every step is the kernel's single rounding).  tables: "reference" -- cos / sin of the fp32 inclinations by torch in fp32, as
        the reference's to_pc_torch takes them -- or "library": in fp64, rounded once to fp32, as rldm_lidar_create builds them (the
        two differ in the last bit of a few beams).  The azimuth's cos / sin are taken in fp64 of the angle in x's dtype (the
        reference's own in fp64, the library's table in fp32).  points (B, W * H, >= 3): take x, y, z from there instead (the device's
        own to_pc_torch output, which removes the libm's exp2f from a comparison).  Differentiable in x through the remainders."""
        B, Cc, W, H = x.shape
        dt, dev = x.dtype, x.device
        gz, gy, gx = (int(g) for g in self.grid_sizes)
        if tables not in ("reference", "library"):
            raise ValueError(f"tables is 'reference' or 'library', not {tables!r}")
        incl = torch.from_numpy(np.ascontiguousarray(self.incl, np.float32))
        if tables == "library":
            incl = incl.double()
        ci, si = torch.cos(incl).float().to(dt).to(dev), torch.sin(incl).float().to(dt).to(dev)
        hgt = torch.from_numpy(np.ascontiguousarray(self.height, np.float32)).to(dt).to(dev)
        azi = (W - 0.5 - torch.arange(0, W, dtype=dt, device=dev)) / W * 2. * torch.pi - torch.pi
        ca, sa = torch.cos(azi.double()).to(dt), torch.sin(azi.double()).to(dt)
        v, f = x[:, 0], x[:, 1]
        if self.log:
            raw = 2 ** (v * 6) - 1
        elif self.inverse:
            raw = 1 / torch.where(v > 1e-4, v, torch.full_like(v, 1e-4))
        else:
            raw = v * self.std + self.mean
        replaced = raw < 0
        r = torch.where(replaced, torch.full_like(raw, float(self.range_fill_value[0])), raw)
        xy = r * ci[None, None, :]
        pz_m = hgt[None, None, :] - r * si[None, None, :]
        px_m, py_m = xy * ca[None, :, None], xy * sa[None, :, None]
        if points is not None:
            p3 = points.to(dt).reshape(B, W, H, -1)
            px_m, py_m, pz_m = p3[..., 0], p3[..., 1], p3[..., 2]
        rng = torch.tensor([float(c) for c in self.pc_range], dtype=dt, device=dev)
        centre, half = (rng[3:] + rng[:3]) / 2, (rng[3:] - rng[:3]) / 2
        coords, touch = [], torch.ones_like(replaced)
        for m, k, g in ((px_m, 0, gx), (py_m, 1, gy), (pz_m, 2, gz)):
            p = (((m - centre[k]) / half[k] + 1) * 0.5) * (g - 1)
            coords.append(p)
            touch = touch & (p > -1) & (p < g)                       # (False for NaN, as the kernel's test)
        fl = [torch.floor(torch.where(touch, p.detach(), torch.zeros_like(p))) for p in coords]
        rem = [torch.where(touch, p, torch.zeros_like(p)) - q for p, q in zip(coords, fl)]
        return dict(v=v, f=f, replaced=replaced, touch=touch, cell=[q.long() for q in fl], rem=rem, tables=(ci, si, ca, sa),
                    half=half, grid=(gx, gy, gz))

    @staticmethod
    def _bev_votes(geo):
        """The 8 votes of every pixel: [(dx, dy, dz, flat cell index (0 where the vote is dropped), in-grid mask, wx, wy, wz)]."""
        gx, gy, gz = geo["grid"]
        (X, Y, Z), (rx, ry, rz) = geo["cell"], geo["rem"]
        out = []
        for dx in (0, 1):
            wx = rx if dx else 1 - rx
            for dy in (0, 1):
                wy = ry if dy else 1 - ry
                for dz in (0, 1):
                    wz = rz if dz else 1 - rz
                    X_, Y_, Z_ = X + dx, Y + dy, Z + dz
                    ok = geo["touch"] & (X_ >= 0) & (X_ < gx) & (Y_ >= 0) & (Y_ < gy) & (Z_ >= 0) & (Z_ < gz)
                    idx = torch.where(ok, (Z_ * gy + Y_) * gx + X_, torch.zeros_like(X_))
                    out.append((dx, dy, dz, idx, ok, wx, wy, wz))
        return out

    def to_voxel_host(self, range_images, return_raw=False, tables="reference"):
        """The reference's to_pc_torch + to_voxel + _splat_points_to_volumes (ldm/dataset.py:13-132, 228-294) in plain torch, on any
        device, in the input's dtype (fp32 or fp64), differentiable in range_images.  Votes outside the volume are dropped (the
        reference adds them to a random voxel with weight 0).  return_raw: -> (voxel, d, S), the accumulators (B, D, H, W) before the
        finalise step.  tables: see _bev_geometry."""
        x = range_images
        if x.dim() != 4 or x.shape[3] != self.H or x.shape[1] < 2:
            raise ValueError(f"range_images must be (B, >= 2, W, {self.H}), got {tuple(x.shape)}")
        B = x.shape[0]
        geo = self._bev_geometry(x, tables=tables)
        gx, gy, gz = geo["grid"]
        nvox = gx * gy * gz
        base = (torch.arange(B, device=x.device) * nvox).reshape(B, 1, 1)
        d = torch.zeros(B * nvox, dtype=x.dtype, device=x.device)
        S = torch.zeros_like(d)
        for _, _, _, idx, ok, wx, wy, wz in self._bev_votes(geo):
            w = torch.where(ok, wx * wy * wz, torch.zeros_like(wx))
            flat = (idx + base).reshape(-1)
            d = d.index_add(0, flat, w.reshape(-1))
            S = S.index_add(0, flat, (w * geo["f"]).reshape(-1))
        d, S = d.reshape(B, gz, gy, gx), S.reshape(B, gz, gy, gx)
        feat = S / d.clamp(min=1e-4)
        vox = torch.cat([torch.log(d + 1) if self.normalize_volume_densities else d, feat], 1)
        return (vox, d, S) if return_raw else vox

    def to_voxel_ordered_host(self, range_images, points=None, tables="library", return_raw=True):
        """rldm_lidar_to_voxel_ordered stated in numpy fp32.  Geometry, in-grid tests and weights are _bev_geometry / _bev_votes in
        fp32 (points, tables: see _bev_geometry; the device's own to_pc_torch output as points removes the log mode's exp2f from a
        comparison).  A vote has the id v = n * 8 + (dx * 4 + dy * 2 + dz), n = w * H + h; it counts when its pixel touches the
        volume, its corner lies inside the grid and w != 0.  Per image and cell, over the cell's counted votes in ascending v:
        d = ((0 + w_1) + w_2) + ..., S the same over w * f -- np.cumsum on fp32, which adds left to right --, +0 in a cell without
        votes.  Then the finalise step: S / max(d, 1e-4) and log(d + 1) or d (numpy's log, not the device's logf).
        -> (voxel (B, 2 D, H, W), d (B, D, H, W), S) as fp32 numpy arrays, or voxel alone."""
        x = torch.as_tensor(np.asarray(range_images.detach().cpu() if torch.is_tensor(range_images) else range_images, np.float32))
        if x.dim() != 4 or x.shape[3] != self.H or x.shape[1] < 2:
            raise ValueError(f"range_images must be (B, >= 2, W, {self.H}), got {tuple(x.shape)}")
        if points is not None:
            points = torch.as_tensor(np.asarray(points.detach().cpu() if torch.is_tensor(points) else points, np.float32))
        B = x.shape[0]
        geo = self._bev_geometry(x, points, tables)
        gx, gy, gz = geo["grid"]
        nvox = gx * gy * gz
        f = geo["f"]
        cell, counted, w, wf = [], [], [], []
        for _, _, _, idx, ok, wx, wy, wz in self._bev_votes(geo):                        # (dx, dy, dz) in the kernel's loop order
            wv = (wx * wy) * wz
            cell.append(idx.reshape(B, -1))
            counted.append((ok & (wv != 0)).reshape(B, -1))
            w.append(wv.reshape(B, -1))
            wf.append((wv * f).reshape(B, -1))
        # (B, N, 8) flattened: position v = n * 8 + (dx * 4 + dy * 2 + dz)
        cell, counted, w, wf = (torch.stack(t, 2).reshape(B, -1).numpy() for t in (cell, counted, w, wf))
        d, S = np.zeros((B, nvox), np.float32), np.zeros((B, nvox), np.float32)
        zero = np.zeros(1, np.float32)
        for b in range(B):
            v = np.flatnonzero(counted[b])                                                # ascending v
            order = v[np.argsort(cell[b][v], kind="stable")]                              # by cell; within a cell still ascending v
            cells, first = np.unique(cell[b][order], return_index=True)
            for c, lo, hi in zip(cells, first, list(first[1:]) + [len(order)]):
                seg = order[lo:hi]
                d[b, c] = np.cumsum(np.concatenate([zero, w[b][seg]]), dtype=np.float32)[-1]
                S[b, c] = np.cumsum(np.concatenate([zero, wf[b][seg]]), dtype=np.float32)[-1]
        d, S = d.reshape(B, gz, gy, gx), S.reshape(B, gz, gy, gx)
        with np.errstate(all="ignore"):
            feat = S / np.maximum(d, np.float32(1e-4))
            dens = np.log(d + np.float32(1)) if self.normalize_volume_densities else d
        vox = np.concatenate([dens, feat], 1).astype(np.float32)
        return (vox, d, S) if return_raw else vox

    def to_voxel_backward_host(self, images, d_raw, S_raw, dvoxel, points=None, return_terms=False, tables="reference"):
        """rldm_lidar_to_voxel_backward stated in torch: the geometry (cells, remainders, in-grid tests) in `images`' dtype by
        _bev_geometry -- the kernel's own fp32 numbers for an fp32 image --, then the two steps in fp64, given the accumulators d_raw,
        S_raw (B, D, H, W): per cell a = gD / (d + 1) [or gD] - [d >= 1e-4] gF S / d^2, e = gF / max(d, 1e-4); per pixel the gather
        over its in-grid votes (weight 0 included) and the chain rule through grid coordinate, point and decoded range.  The 1e-4 is
        the fp32 number the kernels compare with when images are fp32.  -> dimages (B, 2, W, H) fp64; return_terms: also the sum of
        |every product the gather adds| per output element (same shape), what a rounding bound of the device's result scales with.
        points, tables: see _bev_geometry (a comparison with the device passes its points and tables="library")."""
        with torch.no_grad():
            x = images.detach()
            B, Cc, W, H = x.shape
            geo = self._bev_geometry(x, points, tables)
            gx, gy, gz = geo["grid"]
            nvox = gx * gy * gz
            mw = float(np.float32(1e-4)) if x.dtype == torch.float32 else 1e-4
            d, S = d_raw.detach().double().reshape(B, nvox), S_raw.detach().double().reshape(B, nvox)
            g = dvoxel.detach().double().reshape(B, 2, nvox)
            gD, gF = g[:, 0], g[:, 1]
            a1 = gD / (d + 1) if self.normalize_volume_densities else gD
            a2 = torch.where(d >= mw, gF * S / torch.where(d >= mw, d * d, torch.ones_like(d)), torch.zeros_like(d))
            a, e = a1 - a2, gF / d.clamp(min=mw)
            a_abs = a1.abs() + a2.abs()
            f = geo["f"].double()
            zero = torch.zeros_like(f)
            df, dp, df_abs, dp_abs = zero.clone(), [zero.clone() for _ in range(3)], zero.clone(), [zero.clone() for _ in range(3)]
            for dx, dy, dz, idx, ok, wx, wy, wz in self._bev_votes(geo):
                wx, wy, wz = wx.double(), wy.double(), wz.double()
                flat = idx.reshape(B, -1)
                av, ev = (torch.gather(t, 1, flat).reshape(f.shape) for t in (a, e))
                aa = torch.gather(a_abs, 1, flat).reshape(f.shape)
                q, q_abs = av + f * ev, aa + (f * ev).abs()
                m = ok.double()
                df += m * wx * wy * wz * ev
                df_abs += m * (wx * wy * wz * ev).abs()
                for k, (s, ww) in enumerate(((dx, wy * wz), (dy, wx * wz), (dz, wx * wy))):
                    dp[k] += m * (2 * s - 1) * q * ww
                    dp_abs[k] += m * q_abs * ww.abs()
            v = geo["v"].double()
            if self.log:
                drdv = 6 * np.log(2.0) * 2 ** (6 * v)
            elif self.inverse:
                drdv = torch.where(v > mw, -1 / (v * v), torch.zeros_like(v))
            else:
                drdv = torch.full_like(v, float(self.std))
            drdv = torch.where(geo["replaced"], torch.zeros_like(drdv), drdv)
            ci, si, ca, sa = (t.double() for t in geo["tables"])
            half = geo["half"].double()
            k = [0.5 * (n - 1) / half[i] for i, n in enumerate((gx, gy, gz))]
            jac = (k[0] * ci[None, None, :] * ca[None, :, None], k[1] * ci[None, None, :] * sa[None, :, None],
                   (-k[2] * si[None, None, :]).expand(1, W, H))
            dv = (dp[0] * jac[0] + dp[1] * jac[1] + dp[2] * jac[2]) * drdv
            out = torch.stack([dv, df], 1)
            if not return_terms:
                return out
            dv_abs = (dp_abs[0] * jac[0].abs() + dp_abs[1] * jac[1].abs() + dp_abs[2] * jac[2].abs()) * drdv.abs()
            return out, torch.stack([dv_abs, df_abs], 1)

    def filter_points(self, point_cloud, max_depth=90.0):
        """Per image `pc[np.linalg.norm(pc[:, :3], 2, axis=1) < max_depth]`, order kept (ldm/inference.py:177-179).
        Returns (points (B, N, cols) with the kept rows packed to the front, counts (B,) int32), both on device."""
        pc = point_cloud.detach().float().contiguous()
        B, N, cols = pc.shape
        out = torch.empty_like(pc)
        counts = torch.empty((B,), dtype=torch.int32, device=pc.device)
        _lib.check(_lib.lib().rldm_lidar_filter_points(self._handle(), pc.data_ptr(), B, N, cols, float(max_depth),
                                                       out.data_ptr(), counts.data_ptr(), _lib.stream_ptr(pc.device)),
                   "rldm_lidar_filter_points")
        return out, counts

    # ---- f3: in front of the training path -------------------------------------------------------------------
    def get_row_inds(self, pc):
        raise NotImplementedError

    def project(self, pc):
        """`__call__` + `process_miss_value` + `normalize` + the permutes of RangeDataset.__getitem__
        (ldm/dataset.py:159-226, 320-333) in one pass: pc (N, >= 4) device fp32 ->
        dict(jpg=(2, W, H) fp32, mask=(W, H) bool, car_window_mask=(W, H) bool) on the device."""
        if not pc.is_cuda:
            raise RuntimeError("pc must live on the GPU (rangeldm_amd has no CPU path)")
        pc = pc.detach().float().contiguous()
        n, stride = pc.shape
        rows = self.get_row_inds(pc)
        if rows is not None:
            rows = rows.to(torch.int32).contiguous()
        W, H = self.width, self.H
        img = torch.empty((2, W, H), dtype=torch.float32, device=pc.device)
        mask = torch.empty((W, H), dtype=torch.uint8, device=pc.device)
        car = torch.empty((W, H), dtype=torch.uint8, device=pc.device)
        _lib.check(_lib.lib().rldm_lidar_project(self._handle(), pc.data_ptr(), n, stride,
                                                 rows.data_ptr() if rows is not None else None, float(self.min_depth),
                                                 img.data_ptr(), mask.data_ptr(), car.data_ptr(),
                                                 _lib.stream_ptr(pc.device)), "rldm_lidar_project")
        return {"jpg": img, "mask": mask.bool(), "car_window_mask": car.bool()}


def render_u8(images, channel=0):
    """`(images[j].permute(2, 1, 0).clip(0, 1) * 255).astype(uint8)[:, :, channel]` for every j
    (ldm/inference.py:180-183): (B, C, W, H) device fp32 -> (B, H, W) device uint8, the pixels of the 8-bit PNGs."""
    if not images.is_cuda:
        raise RuntimeError("images must live on the GPU (rangeldm_amd has no CPU path)")
    x = images.detach().float().contiguous()
    B, Cc, W, H = x.shape
    out = torch.empty((B, H, W), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().rldm_render_u8(x.data_ptr(), B, Cc, W, H, int(channel), out.data_ptr(),
                                         _lib.stream_ptr(x.device)), "rldm_render_u8")
    return out


# Per-beam calibration of the two sensors (data, ldm/kitti360_range_image.py:19-48 / ldm/nuscenes_range_image.py:20-35):
# mounting height offset [m] and zenith angle [rad] of every laser, top beam first.
_KITTI_HEIGHT = (
    0.20966667, 0.2092, 0.2078, 0.2078, 0.2078, 0.20733333, 0.20593333, 0.20546667, 0.20593333, 0.20546667, 0.20453333,
    0.205, 0.2036, 0.20406667, 0.2036, 0.20313333, 0.20266667, 0.20266667, 0.20173333, 0.2008, 0.2008, 0.2008, 0.20033333,
    0.1994, 0.20033333, 0.19986667, 0.1994, 0.1994, 0.19893333, 0.19846667, 0.19846667, 0.19846667, 0.12566667, 0.1252,
    0.1252, 0.12473333, 0.12473333, 0.1238, 0.12333333, 0.1238, 0.12286667, 0.1224, 0.12286667, 0.12146667, 0.12146667,
    0.121, 0.12053333, 0.12053333, 0.12053333, 0.12006667, 0.12006667, 0.1196, 0.11913333, 0.11866667, 0.1182, 0.1182,
    0.1182, 0.11773333, 0.11726667, 0.11726667, 0.1168, 0.11633333, 0.11633333, 0.1154)
_KITTI_ZENITH = (
    0.03373091, 0.02740409, 0.02276443, 0.01517224, 0.01004049, 0.00308099, -0.00155868, -0.00788549, -0.01407172,
    -0.02103122, -0.02609267, -0.032068, -0.03853542, -0.04451074, -0.05020488, -0.0565317, -0.06180405, -0.06876355,
    -0.07361411, -0.08008152, -0.08577566, -0.09168069, -0.09793721, -0.10398284, -0.11052055, -0.11656618, -0.12219002,
    -0.12725147, -0.13407038, -0.14067839, -0.14510716, -0.15213696, -0.1575499, -0.16711043, -0.17568678, -0.18278688,
    -0.19129293, -0.20247031, -0.21146846, -0.21934183, -0.22763699, -0.23536977, -0.24528179, -0.25477201, -0.26510582,
    -0.27326038, -0.28232882, -0.28893683, -0.30004392, -0.30953414, -0.31993824, -0.32816311, -0.33723155, -0.34447224,
    -0.352908, -0.36282001, -0.37216965, -0.38292524, -0.39164219, -0.39895318, -0.40703745, -0.41835542, -0.42777535,
    -0.43621111)
_NUSC_HEIGHT = (
    -0.00216031, -0.00098729, -0.00020528, 0.00174976, 0.0044868, -0.00294233, -0.00059629, -0.00020528, 0.00174976,
    -0.00294233, -0.0013783, 0.00018573, 0.00253177, -0.00098729, 0.00018573, 0.00096774, -0.00411535, -0.0013783,
    0.00018573, 0.00018573, -0.00294233, -0.0013783, -0.00098729, -0.00020528, 0.00018573, 0.00018573, 0.00018573,
    -0.00020528, 0.00018573, 0.00018573, 0.00018573, 0.00018573)
_NUSC_ZENITH = (
    1.86705767e-01, 1.63245357e-01, 1.39784946e-01, 1.16324536e-01, 9.28641251e-02, 7.01857283e-02, 4.67253177e-02,
    2.32649071e-02, -1.95503421e-04, -2.28739003e-02, -4.63343109e-02, -6.97947214e-02, -9.32551320e-02, -1.15933529e-01,
    -1.39393939e-01, -1.62854350e-01, -1.85532747e-01, -2.08993157e-01, -2.32453568e-01, -2.55913978e-01, -2.78592375e-01,
    -3.02052786e-01, -3.25513196e-01, -3.48973607e-01, -3.72434018e-01, -3.95894428e-01, -4.19354839e-01, -4.42033236e-01,
    -4.65493646e-01, -4.88954057e-01, -5.12414467e-01, -5.35874878e-01)


class point_cloud_to_range_image_KITTI(point_cloud_to_range_image):
    """64-beam KITTI-360 sensor; beam of a return = closest inclination (ldm/kitti360_range_image.py:51-61), found
    inside the projection kernel."""

    def __init__(self, **kwargs) -> None:
        self.height = np.array(_KITTI_HEIGHT, dtype=np.float32)
        self.zenith = np.array(_KITTI_ZENITH, dtype=np.float32)
        self.incl = -self.zenith
        self.H = 64
        super().__init__(**kwargs)

    def get_row_inds(self, pc):
        return None                     # nearest-inclination search runs on the device


class point_cloud_to_range_image_nuScenes(point_cloud_to_range_image):
    """32-beam nuScenes sensor; the sweep carries the ring index in column 4 (ldm/nuscenes_range_image.py:43-45) and
    returns closer than 2 m are dropped (:37-41)."""

    def __init__(self, **kwargs) -> None:
        self.height = np.array(_NUSC_HEIGHT, dtype=np.float32)
        self.zenith = np.array(_NUSC_ZENITH, dtype=np.float32)
        self.incl = -self.zenith
        self.H = 32
        super().__init__(**kwargs)
        self.min_depth = 2.0

    def get_row_inds(self, pc):
        return 31 - pc[:, 4].to(torch.int32)


class point_cloud_to_range_image_tables(point_cloud_to_range_image):
    """A sensor given by its tables: height [m] and incl [rad, positive downwards] per beam, top beam first -- what
    sensor.estimate_sensor returns for a sensor without shipped constants.  `height` may also be a sensor.SensorTables (or any
    object with .height and .incl), with `incl` left out.  Beam of a return = closest inclination, found inside the
    projection kernel, as for KITTI-360."""

    def __init__(self, height, incl=None, **kwargs) -> None:
        if incl is None:
            height, incl = height.height, height.incl
        self.height = np.array(height, dtype=np.float32).reshape(-1)
        self.incl = np.array(incl, dtype=np.float32).reshape(-1)
        if self.height.shape != self.incl.shape or not 1 <= len(self.incl) <= 4096:
            raise ValueError("height and incl must be two vectors of 1 .. 4096 beams")
        self.zenith = -self.incl
        self.H = len(self.incl)
        super().__init__(**kwargs)

    def get_row_inds(self, pc):
        return None                     # nearest-inclination search runs on the device
