"""Host-side driver of the hot path: mirrors the phase sequence of
HDK_AdaptiveViscosity::solveGasSubclass between cpp:418 and cpp:653, calling only the C ABI
(include/avs.h).  Buffers are numpy arrays (host) or torch tensors (host or HBM); torch is used
for device memory and streams only.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import capi


class ViscositySolve:
    """One adaptive-viscosity solve on one MI355X.

    Typical use (same order as the reference):
        s = ViscositySolve(res, dx, dt, levels)          # cpp:126-275
        s.set_pyramid(pyramid); s.set_scene_fields(scene) # outputs of cpp:233-416
        info = s.assemble()                               # cpp:418-594, 613-614
        sol = s.solve(tol, max_iters)                     # cpp:618-630
        x = s.solution()                                  # viscositySolution, consumed by cpp:661-707
    """

    def __init__(self, res, dx, dt, levels, use_enhanced_gradients=True, device=0, stream=None, field_res=None, precision=capi.PRECISION_F64,
                 probe=False):
        """`res`: octree (power-of-two) level-0 resolution; `field_res`: resolution of the simulation grid the scalar
        fields live on when HDK_OctreeGrid::init had to pad it (oct.cpp:13-24); None = res.  probe=True: the context lives in
        libavs_probe.so (the same sources + the measurement entries of include/avs_probe.h: bench_spmv ...) -- tools and tests only."""
        self.lib = capi.load(probe=probe)
        self.res = tuple(int(r) for r in res)
        fr = tuple(int(r) for r in field_res) if field_res is not None else (0, 0, 0)
        d = capi.Desc(self.res[0], self.res[1], self.res[2], float(dx), float(dt), int(levels),
                      int(bool(use_enhanced_gradients)), int(device), C.c_void_p(stream or 0), fr[0], fr[1], fr[2], int(precision))
        h = C.c_void_p()
        capi.check(self.lib.avs_create(C.byref(d), C.byref(h)))
        self.h = h
        self.levels = int(levels)
        self.precision = int(precision)
        self.device = int(device)
        self.counts = None
        self.field_res = tuple(fr[a] or self.res[a] for a in range(3))

    def close(self):
        if getattr(self, "h", None):
            self.lib.avs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inputs ---------------------------------------------------------------------------
    def set_labels(self, level, labels):
        p, where = capi.ptr_of(labels)
        capi.check(self.lib.avs_set_labels(self.h, level, p, where))

    def set_index_field(self, kind, level, axis, idx):
        p, where = capi.ptr_of(idx)
        capi.check(self.lib.avs_set_index_field(self.h, kind, level, axis, p, where))

    def set_dof_counts(self, nv, ne, nc):
        capi.check(self.lib.avs_set_dof_counts(self.h, nv, ne, nc))
        self.counts = (int(nv), int(ne), int(nc))

    def _field_lattice(self, kind, axis, res):
        """(nz, ny, nx) of a level-0 scalar field's lattice on a grid of resolution `res` (x, y, z)."""
        r = list(res)
        if kind in (capi.FIELD_FACE_WEIGHTS, capi.FIELD_VELOCITY, capi.FIELD_SOLID_VELOCITY):
            r[axis] += 1
        elif kind == capi.FIELD_EDGE_WEIGHTS:
            r = [r[b] + (1 if b != axis else 0) for b in range(3)]
        return (r[2], r[1], r[0])

    def set_field(self, kind, axis=0, data=None, const=0.0):
        if data is not None and self.field_res != self.res:
            # the library expects the SIMULATION grid's lattice; crop arrays given on the padded octree lattice
            full, want = self._field_lattice(kind, axis, self.res), self._field_lattice(kind, axis, self.field_res)
            if tuple(data.shape) == full:
                data = data[:want[0], :want[1], :want[2]]
                data = data.contiguous() if hasattr(data, "contiguous") else np.ascontiguousarray(data)
            assert tuple(data.shape) == want, (tuple(data.shape), want)
        p, where = capi.ptr_of(data)
        capi.check(self.lib.avs_set_scalar_field(self.h, kind, axis, p, float(const), where))

    def set_pyramid(self, pyr):
        """Upload a prepass.Pyramid (labels, index pyramids, counts, integration weights)."""
        def c(t, dtype):
            if isinstance(t, np.ndarray):
                return np.ascontiguousarray(t, dtype=dtype)
            import torch
            tdt = {np.int8: torch.int8, np.int32: torch.int32, np.float32: torch.float32}[dtype]
            return t.to(tdt).contiguous()
        for l in range(pyr.levels):
            self.set_labels(l, c(pyr.labels[l], np.int8))
            for a in range(3):
                self.set_index_field(capi.INDEX_VELOCITY, l, a, c(pyr.vidx[l][a], np.int32))
                self.set_index_field(capi.INDEX_EDGE, l, a, c(pyr.eidx[l][a], np.int32))
            self.set_index_field(capi.INDEX_CENTER, l, 0, c(pyr.cidx[l], np.int32))
        self.set_dof_counts(pyr.n_velocity, pyr.n_edge, pyr.n_center)
        self.set_field(capi.FIELD_CENTER_WEIGHTS, 0, c(pyr.center_weights, np.float32))
        for a in range(3):
            self.set_field(capi.FIELD_EDGE_WEIGHTS, a, c(pyr.edge_weights[a], np.float32))
            self.set_field(capi.FIELD_FACE_WEIGHTS, a, c(pyr.face_weights[a], np.float32))

    def set_scene_fields(self, scene):
        """viscosity / density / velocity / solid velocity of a scenes.Scene."""
        def put(kind, axis, v):
            if isinstance(v, (int, float)):
                self.set_field(kind, axis, None, float(v))
            else:
                self.set_field(kind, axis, v.contiguous() if hasattr(v, "contiguous") else np.ascontiguousarray(v))
        put(capi.FIELD_VISCOSITY, 0, scene.viscosity)
        put(capi.FIELD_DENSITY, 0, scene.density)
        for a in range(3):
            put(capi.FIELD_VELOCITY, a, scene.velocity[a])
            if scene.solid_velocity is None:
                self.set_field(capi.FIELD_SOLID_VELOCITY, a, None, 0.0)
            else:
                put(capi.FIELD_SOLID_VELOCITY, a, scene.solid_velocity[a])

    def set_solver_option(self, option, value):
        """avs_set_solver_option: e.g. (capi.OPTION_PRECONDITIONER, capi.PRECONDITIONER_NONE) = plain CG (cpp:638-642)."""
        capi.check(self.lib.avs_set_solver_option(self.h, int(option), int(value)))
        if int(option) == capi.OPTION_F32_VECTORS:
            self.f32_vectors_off = int(value) == 0
            self.f32_vectors_set = int(value) >= 0     # an explicit option overrides AVS_F32_VECTORS in the environment

    # ---- hot path -------------------------------------------------------------------------
    def build_stencils(self):
        capi.check(self.lib.avs_build_stencils(self.h))

    def build_initial_guess(self):
        capi.check(self.lib.avs_build_initial_guess(self.h))

    def build_system(self):
        capi.check(self.lib.avs_build_system(self.h))

    def assemble(self):
        info = capi.AssemblyInfo()
        capi.check(self.lib.avs_assemble(self.h, C.byref(info)))
        self.ainfo = info
        return info

    def solve(self, tol=1e-3, max_iters=2500):
        info = capi.SolveInfo()
        capi.check(self.lib.avs_solve(self.h, float(tol), int(max_iters), C.byref(info)))
        return info

    # ---- multi-GPU ---------------------------------------------------------------------------
    def dist_init(self, rank, world):
        """RCCL communicator: the unique id is made on rank 0 and broadcast with torch.distributed."""
        import torch
        import torch.distributed as dist
        ident = torch.zeros(capi.UNIQUE_ID_BYTES, dtype=torch.uint8)
        if rank == 0:
            buf = (C.c_uint8 * capi.UNIQUE_ID_BYTES)()
            capi.check(self.lib.avs_dist_get_unique_id(buf))
            ident = torch.tensor(list(buf), dtype=torch.uint8)
        dev = torch.device("cuda", torch.cuda.current_device())
        t = ident.to(dev)
        dist.broadcast(t, src=0)
        raw = bytes(t.cpu().tolist())
        buf = (C.c_uint8 * capi.UNIQUE_ID_BYTES).from_buffer_copy(raw)
        capi.check(self.lib.avs_dist_init(self.h, buf, rank, world))

    def dist_init_hosted(self, rank, world):
        """Hosted group (no RCCL communicator): the host program moves the comm-block blobs; here torch.distributed (any backend)
        all-gathers them after every distributed assembly / partition (`_hosted_connect`)."""
        capi.check(self.lib.avs_dist_init_hosted(self.h, rank, world))
        self._hosted = (rank, world)

    def _hosted_connect(self):
        import torch
        import torch.distributed as dist
        rank, world = self._hosted
        blob = (C.c_uint8 * capi.DIST_BLOB_BYTES)()
        capi.check(self.lib.avs_dist_export_blob(self.h, blob))
        mine = torch.tensor(list(bytes(blob)), dtype=torch.uint8)
        if dist.get_backend() == "nccl":
            mine = mine.to(torch.device("cuda", torch.cuda.current_device()))
        allb = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allb, mine)
        raw = b"".join(bytes(t.cpu().tolist()) for t in allb)
        buf = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
        capi.check(self.lib.avs_dist_import_blobs(self.h, buf))   # maps the peers' blocks and runs the transport self-test

    def dist_init_local(self, group, rank):
        capi.check(self.lib.avs_dist_init_local(self.h, group, rank))

    def dist_partition(self, cut_axis=-1):
        capi.check(self.lib.avs_dist_partition(self.h, cut_axis))
        sz = capi.PlanSizes()
        capi.check(self.lib.avs_dist_get_plan_sizes(self.h, C.byref(sz)))
        self.plan_sizes = sz
        self.local_spmv_bytes = 12 * sz.nnz_local + 4 * (sz.n_own + 1) + 16 * sz.n_own
        ti, tb = C.c_int32(), C.c_int32()
        capi.check(self.lib.avs_dist_get_overlap_tiles(self.h, C.byref(ti), C.byref(tb)))
        self.overlap_tiles = (ti.value, tb.value)
        return sz

    def dist_assemble(self, cut_axis=-1):
        """Distributed assembly: this rank assembles only the rows of its slab (instead of assemble + dist_partition)."""
        info = capi.AssemblyInfo()
        capi.check(self.lib.avs_dist_assemble(self.h, cut_axis, C.byref(info)))
        sz = capi.PlanSizes()
        capi.check(self.lib.avs_dist_get_plan_sizes(self.h, C.byref(sz)))
        self.plan_sizes = sz
        self.local_spmv_bytes = 12 * sz.nnz_local + 4 * (sz.n_own + 1) + 16 * sz.n_own
        ti, tb = C.c_int32(), C.c_int32()
        capi.check(self.lib.avs_dist_get_overlap_tiles(self.h, C.byref(ti), C.byref(tb)))
        self.overlap_tiles = (ti.value, tb.value)
        if getattr(self, "_hosted", None) and self._hosted[1] > 1:
            self._hosted_connect()
        return info

    def dist_bind_prepass(self, prepass, cuts, cut_axis=-1):
        """The pre-pass object's next runs are slab-local: this rank's window of the lattices only, global ids through one all-reduce of
        per-tile counts over this context's group (avs_dist_bind_prepass).  cuts: world + 1 fine-cell coordinates, or None (off)."""
        if cuts is None:
            capi.check(self.lib.avs_dist_bind_prepass(self.h, prepass.h, cut_axis, None))
            return
        c = np.ascontiguousarray(cuts, np.int32)
        capi.check(self.lib.avs_dist_bind_prepass(self.h, prepass.h, cut_axis, c.ctypes.data))

    def dist_cuts(self, world, which=0):
        """(cut_axis, cuts[world + 1]) of the last avs_dist_assemble (which = 0) / what its weights suggest for the next frame (1)."""
        cuts = np.empty(world + 1, np.int32)
        ax = C.c_int32()
        capi.check(self.lib.avs_dist_get_cuts(self.h, which, C.byref(ax), cuts.ctypes.data))
        return ax.value, cuts

    def dist_solve(self, tol=1e-3, max_iters=2500):
        info = capi.SolveInfo()
        capi.check(self.lib.avs_dist_solve(self.h, float(tol), int(max_iters), C.byref(info)))
        return info

    def dist_comm_info(self):
        """dict form of avs_dist_info (transport, RCCL rank count, launches / collectives per iteration)."""
        di = capi.DistInfo()
        capi.check(self.lib.avs_dist_get_info(self.h, C.byref(di)))
        return {"world_size": int(di.world_size), "rccl_ranks": int(di.rccl_ranks),
                "transport": {0: "rccl", 1: "direct"}.get(int(di.transport), str(di.transport)),
                "graph_replay": bool(di.graph_replay), "launches_per_iteration": int(di.launches_per_iteration),
                "rccl_calls_per_iteration": int(di.collectives_per_iteration),
                "selftest_rounds": int(di.selftest_rounds), "selftest_bad_entries": int(di.selftest_bad_entries),
                "paranoid": bool(di.paranoid)}

    def dist_solution(self):
        n = self.info().n_velocity
        x = np.empty(n, np.float64)
        capi.check(self.lib.avs_dist_get_solution(self.h, x.ctypes.data, n, capi.MEM_HOST))
        return x

    def dof_table(self, kind=capi.INDEX_VELOCITY):
        i = self.info()
        n = {capi.INDEX_VELOCITY: i.n_velocity, capi.INDEX_EDGE: i.n_edge, capi.INDEX_CENTER: i.n_center}[kind]
        t = np.empty((n, 4), np.int32)
        capi.check(self.lib.avs_get_dof_table(self.h, kind, t.ctypes.data, capi.MEM_HOST))
        return t

    def bench_spmv(self, variant=0, repeats=100):
        """mean time of one launch of the solver's SpMV (ms); checks y against the plain CSR kernel bit for bit.  Probe library only."""
        if not hasattr(self.lib, "avs_bench_spmv") or self.lib is not capi.load(probe=True):
            raise RuntimeError("bench_spmv is a measurement entry of libavs_probe.so: create the solver with probe=True")
        ms = C.c_double()
        capi.check(self.lib.avs_bench_spmv(self.h, variant, repeats, C.byref(ms)))
        return ms.value

    def matrix_format(self):
        """Storage form the solver's SpMV streams (12 / 6 / 4 bytes per non-zero), see avs_matrix_format."""
        fmt = capi.MatrixFormat()
        capi.check(self.lib.avs_get_matrix_format(self.h, C.byref(fmt)))
        return fmt

    def runs_float_vectors(self, info=None):
        """True when a solve of this context iterates on float vectors (avs_pcg_f32.inl): AVS_PRECISION_F32, not switched off by
        AVS_OPTION_F32_VECTORS / AVS_F32_VECTORS=0, and -- given the avs_solve_info of a solve that ran -- not taken by the CU-resident
        loop (which iterates in fp64 on the float system).  Derived from what ran, not from the precision alone."""
        if getattr(self, "precision", 0) != capi.PRECISION_F32 or getattr(self, "f32_vectors_off", False):
            return False
        env = os.environ.get("AVS_F32_VECTORS")
        if env is not None and env.strip() not in ("", "-1") and int(env) == 0 and not getattr(self, "f32_vectors_set", False):
            return False
        return not (info is not None and int(getattr(info, "resident", 0)))

    def spmv_kernel_name(self, info=None):
        fmt = self.matrix_format()
        bpn, tab = int(fmt.bytes_per_nonzero), int(fmt.value_table_size)
        if self.runs_float_vectors(info):   # the float-vector loop (avs_pcg_f32.inl)
            if int(getattr(fmt, "brick_tiles", 0)):
                return (f"k_spmv_brick<DOT,{'VC,' if int(fmt.brick_value_codes) else ''}float> (brick-structured form, float vectors: {int(fmt.brick_tiles)} tiles, "
                        f"{int(fmt.brick_pattern_rows)} rows as {int(fmt.brick_patterns)} geometric row patterns, x of a brick + halo as floats in LDS; {tab}-entry dictionary; brick-major system)")
            return "k_f32_spmv_csr<DOT> (float vectors: column + value code streamed, float products parked in LDS; brick-major system)"
        # a mixed-precision loop ran (avs_pcg_mixed.inl, or the partitioned loops with AVS_OPTION_DIST_MIXED_PRECISION): an fp64 context
        # iterates on float vectors in no other way (a solve that converged before its first update reports no updates)
        if int(getattr(fmt, "float_vectors", 0)) and (int(getattr(fmt, "reliable_updates", 0)) or getattr(self, "precision", 0) != capi.PRECISION_F32):
            if int(getattr(fmt, "brick_tiles", 0)):
                return (f"k_spmv_brick<DOT,{'VC,' if int(fmt.brick_value_codes) else ''}float,double> (brick-structured form, float vectors, fp64 values and row sums: "
                        f"{int(fmt.brick_tiles)} tiles, {int(fmt.brick_pattern_rows)} rows as {int(fmt.brick_patterns)} geometric row patterns; {tab}-entry dictionary; "
                        f"mixed-precision loop, {int(fmt.reliable_updates)} fp64 residual updates in the last solve; brick-major system)")
            return "k_f32_spmv_csr<DOT,double> (float vectors, fp64 values and row sums; mixed-precision loop; brick-major system)"
        ltab = "LTAB" if 0 < tab <= 2048 else "GTAB"
        cw = int(fmt.column_windows)
        if int(getattr(fmt, "brick_tiles", 0)):
            return (f"k_spmv_brick<DOT> (brick-structured form: {int(fmt.brick_tiles)} tiles, {int(fmt.brick_pattern_rows)} rows as "
                    f"{int(fmt.brick_patterns)} geometric row patterns (8 B per row), x of a brick + halo in LDS, the other rows as 4-B words; "
                    f"{tab}-entry dictionary; brick-major system)")
        if int(fmt.tile_local_tables):
            form = ("4 B/nnz: tile-local value code | window slot | offset in one word" if cw else
                    "6 B/nnz: 2-B tile-local value codes + int32 column")
            return (f"k_spmv_vi2<512,4096,DOT,WIN=512,TLT=1024{',CWIN' if cw else ''}> ({form}; one value dictionary per 512-row tile "
                    f"staged in LDS, {tab} table entries in total; brick-major system)")
        if cw:
            return (f"k_spmv_vi2<512,4096,DOT,{ltab},WIN=512,CWIN> (4 B/nnz: value code | window slot | offset in one word, "
                    f"{tab}-entry dictionary; brick-major system)")
        return {4: f"k_spmv_vi2<512,4096,DOT,{ltab},PACK,WIN=512> (4 B/nnz packed code|column, brick-major system)",
                6: f"k_spmv_vi2<512,4096,DOT,{ltab},WIN=512> (6 B/nnz value-indexed, brick-major system)",
                12: "k_spmv_tile<512,4096,DOT,VEC,NT> (12 B/nnz, brick-major system)"}.get(bpn, f"{bpn} B/nnz")

    # ---- outputs (numpy, host) ------------------------------------------------------------
    def info(self):
        info = capi.AssemblyInfo()
        capi.check(self.lib.avs_get_assembly_info(self.h, C.byref(info)))
        return info

    def solution(self):
        n = self.info().n_velocity
        x = np.empty(n, np.float64)
        capi.check(self.lib.avs_get_solution(self.h, x.ctypes.data, n, capi.MEM_HOST))
        return x

    def set_solution(self, x):
        """hand the context a solution vector (numpy float64 / torch float64, reference numbering) for the transfer"""
        px, wx = capi.ptr_of(x)
        capi.check(self.lib.avs_set_solution(self.h, px, len(x), wx))

    def initial_guess(self):
        n = self.info().n_velocity
        x = np.empty(n, np.float64)
        capi.check(self.lib.avs_get_initial_guess(self.h, x.ctypes.data, n, capi.MEM_HOST))
        return x

    def csr(self):
        i = self.info()
        rp = np.empty(i.n_velocity + 1, np.int32)
        col = np.empty(i.nnz, np.int32)
        val = np.empty(i.nnz, np.float64)
        rhs = np.empty(i.n_velocity, np.float64)
        capi.check(self.lib.avs_get_csr(self.h, rp.ctypes.data, col.ctypes.data, val.ctypes.data,
                                        rhs.ctypes.data, capi.MEM_HOST))
        return rp, col, val, rhs

    def _stencils(self, fn, ns, nw, cap, bcap):
        cnt = np.empty(ns, np.int32); idx = np.empty((cap, ns), np.int32)
        coef = np.empty((cap, ns), np.float64); bcnt = np.empty(ns, np.int32)
        bval = np.empty((bcap, ns), np.float64); w = np.empty(nw, np.float64)
        capi.check(fn(self.h, cnt.ctypes.data, idx.ctypes.data, coef.ctypes.data, bcnt.ctypes.data,
                      bval.ctypes.data, w.ctypes.data, capi.MEM_HOST))
        return dict(cnt=cnt, idx=idx, coef=coef, bcnt=bcnt, bval=bval, weight=w)

    # ---- post-solve transfer (cpp:655-707) -------------------------------------------------
    def set_regular_index_field(self, axis, idx):
        p, where = capi.ptr_of(idx)
        capi.check(self.lib.avs_set_regular_index_field(self.h, axis, p, where))

    def transfer_to_regular_grid(self):
        """Regular MAC-grid velocity (3 fp32 face grids of the simulation grid, host) after the solve."""
        nx, ny, nz = self.field_res
        outs = [np.empty((nz, ny, nx + 1), np.float32), np.empty((nz, ny + 1, nx), np.float32),
                np.empty((nz + 1, ny, nx), np.float32)]
        capi.check(self.lib.avs_transfer_to_regular_grid(self.h, outs[0].ctypes.data, outs[1].ctypes.data,
                                                         outs[2].ctypes.data, capi.MEM_HOST))
        return outs

    def transfer_to_regular_grid_in_place(self, velocity):
        """In-place form (what the reference does to `vel`, cpp:655-707): `velocity` = three DEVICE tensors that hold the field given to
        set_scalar_field(FIELD_VELOCITY); only the faces the transfer changes are written."""
        ptrs = [capi.ptr_of(v) for v in velocity]
        if any(w != capi.MEM_DEVICE for _, w in ptrs):
            raise ValueError("the in-place transfer updates device arrays")
        capi.check(self.lib.avs_transfer_to_regular_grid_in_place(self.h, ptrs[0][0], ptrs[1][0], ptrs[2][0]))

    def node_grid(self, level):
        nx, ny, nz = (r >> level for r in self.res)
        shp = (nz + 1, ny + 1, nx + 1)
        lab = np.empty(shp, np.int8)
        v = [np.empty(shp, np.float32) for _ in range(3)]
        capi.check(self.lib.avs_get_node_grid(self.h, level, lab.ctypes.data, v[0].ctypes.data, v[1].ctypes.data,
                                              v[2].ctypes.data, capi.MEM_HOST))
        return lab, v

    def sample_velocity(self, points, origin=None):
        """The solved octree velocity at arbitrary points (avs_sample_velocity; interpSPGrid, interp.cpp:660-845).  `points`: (N, 3) float32,
        world units -- a numpy array (host path) or a torch tensor on the context's device (device path); origin: world position of the
        grid's lower corner (None = 0, 0, 0).  Returns (velocity (N, 3) float32, inside (N,) uint8) of the same kind; points outside the
        grid or under no ACTIVE cell get velocity 0 and inside 0."""
        org = None if origin is None else np.ascontiguousarray(origin, np.float64).reshape(3)
        po = None if org is None else org.ctypes.data
        if isinstance(points, np.ndarray):
            pts = np.ascontiguousarray(points, np.float32)
            if pts.ndim != 2 or pts.shape[1] != 3:
                raise ValueError("points must have shape (N, 3)")
            vel = np.empty(pts.shape, np.float32)
            inside = np.empty(pts.shape[0], np.uint8)
            capi.check(self.lib.avs_sample_velocity(self.h, pts.shape[0], pts.ctypes.data, po, vel.ctypes.data, inside.ctypes.data, capi.MEM_HOST))
            return vel, inside
        import torch
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError("points must have shape (N, 3)")
        if not points.is_cuda:
            raise ValueError("a torch tensor of points must live on the context's device (host points: pass a numpy array)")
        pts = points.to(torch.float32).contiguous()
        vel = torch.empty_like(pts)
        inside = torch.empty(pts.shape[0], dtype=torch.uint8, device=pts.device)
        # the library works on the context's stream: order it after the caller's work on torch's current stream, and torch's after it
        torch.cuda.current_stream(pts.device).synchronize()
        capi.check(self.lib.avs_sample_velocity(self.h, pts.shape[0], pts.data_ptr(), po, vel.data_ptr(), inside.data_ptr(), capi.MEM_DEVICE))
        return vel, inside

    def octree_cells(self, origin=None, device_arrays=False):
        """The ACTIVE cells of the label pyramid as points (avs_get_octree_cells; outputOctreeGeometry, oct.cpp:245-308), in the reference's
        sweep order.  Returns position (n, 3) float32 (cell centres, world units; origin: the grid's lower corner, None = 0, 0, 0),
        pscale (n,) float32 (the level's voxel size), level (n,) int32, ijk (n, 3) int32 and per_level (MAX_LEVELS,) int64: NumPy arrays,
        or with device_arrays=True torch tensors on the context's device, written there by the kernel (they go straight into
        sample_velocity).  Needs labels only: no assembly, no solve."""
        return _octree_cells(self.lib.avs_get_octree_cells, self.h, origin, device_arrays, self.device)

    def check_octree(self, what=capi.CHECK_LABELS | capi.CHECK_VELOCITY_INDICES):
        """Is the pyramid the context holds one the hot path is defined for?  (avs_check_octree: the reference's debug invariants,
        oct.cpp:984-1304 and cpp:2896-2999, on the device.)  what: capi.CHECK_LABELS (needs labels), capi.CHECK_VELOCITY_INDICES (needs
        the velocity index pyramid and the dof counts too), or both.  Returns an OctreeCheck."""
        return _check_octree(self.lib.avs_check_octree, self.h, what)

    def check_stress_indices(self, what=capi.CHECK_EDGE_INDICES | capi.CHECK_CENTER_INDICES):
        """Are the edge and centre stress index pyramids the context holds ones the hot path is defined for?  (avs_check_stress_indices:
        the reference's debug invariants, cpp:3001-3298, on the device.)  what: capi.CHECK_EDGE_INDICES (needs labels, the velocity and
        edge index pyramids and the dof counts), capi.CHECK_CENTER_INDICES (the centre index pyramid too), or both.  Returns a
        StressCheck."""
        return _check_stress_indices(self.lib.avs_check_stress_indices, self.h, what)

    def check_system(self, what=capi.CSR_CHECK_ALL, symmetry_tolerance=0.0):
        """Is the assembled system one the solve is defined for?  (avs_check_system: the rules of avs_check_csr on the context's
        reference-numbered matrix, its right-hand side and the initial guess, in place.)  Needs assemble(); changes nothing a later
        solve reads.  Returns a CsrCheck: asymmetric_entries and max_abs_asymmetry say how far the assembled A is from bitwise
        symmetric."""
        rep = capi.CsrCheck()
        capi.check(self.lib.avs_check_system(self.h, int(what), float(symmetry_tolerance), C.byref(rep)))
        return _csr_check(rep)

    def check_solution(self, which=capi.CHECK_OF_SOLUTION, residual=False, device_arrays=False):
        """Did x solve the assembled system?  (avs_check_solution: the true residual b - A x in fp64 from the context's reference-numbered
        CSR, in place, whatever loop and storage form produced x.)  which: capi.CHECK_OF_SOLUTION (needs solve / set_solution) or
        capi.CHECK_OF_INITIAL_GUESS.  Returns a SolutionCheck; with residual=True its .residual holds every r_i (a NumPy array, or with
        device_arrays=True a torch tensor on the context's device).  Changes nothing a later solve reads."""
        rep = capi.SolutionCheck()
        if not residual:
            capi.check(self.lib.avs_check_solution(self.h, int(which), None, C.byref(rep), capi.MEM_HOST))
            return _solution_check(rep, None)
        n = int(self.info().n_velocity)
        if not device_arrays:
            out = np.empty(n, np.float64)
            capi.check(self.lib.avs_check_solution(self.h, int(which), out.ctypes.data, C.byref(rep), capi.MEM_HOST))
            return _solution_check(rep, out)
        import torch
        dev = torch.device("cuda", self.device)
        out = torch.empty(n, dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()   # (the stream rules of octree_cells)
        capi.check(self.lib.avs_check_solution(self.h, int(which), out.data_ptr(), C.byref(rep), capi.MEM_DEVICE))
        torch.cuda.synchronize(dev)
        return _solution_check(rep, out)

    def estimate_spectrum(self, op=capi.SPECTRUM_OF_JACOBI, start=capi.SPECTRUM_START_RESIDUAL, steps=32, tolerance=1e-3, scale=False, basis=False,
                          device_arrays=False):
        """Why does the solve take the iterations it takes?  (avs_estimate_spectrum: `steps` Lanczos steps in fp64 on D^-1/2 A D^-1/2 --
        op=capi.SPECTRUM_OF_MATRIX: on A -- from the context's reference-numbered CSR, in place, started from the scaled initial residual
        or from the hash vector.)  Returns a Spectrum: lambda_min / lambda_max with their error bounds, gershgorin_max,
        condition_estimate (a lower bound), iteration_bound for `tolerance`, indefinite, and the arrays alpha, beta, ritz; with scale=True /
        basis=True also .scale (n) and .basis (steps + 1 rows of n: row j = v_j) as NumPy arrays, or with device_arrays=True as torch
        tensors on the context's device.  Changes nothing a later solve reads."""
        n = int(self.info().n_velocity)
        return _estimate(lambda *a: self.lib.avs_estimate_spectrum(self.h, *a), n, op, start, steps, tolerance, scale, basis,
                         self.device if device_arrays else None)

    def strain_rates(self, which=capi.RATES_OF_SOLUTION, device_arrays=False):
        """The deformation of a velocity (avs_get_strain_rates): the rate of every edge stencil (eps_bc at an edge of axis a) and of every
        centre list (du_a/dx_a; list id = cell id + n_center * axis), the shear rate sqrt(2 eps:eps) of every ACTIVE cell (by centre id)
        and the summary (counters, dissipations, maxima).  which: capi.RATES_OF_SOLUTION (needs solve / set_solution) or
        capi.RATES_OF_INITIAL_GUESS (needs build_stencils + build_initial_guess only).  Returns a StrainRates of NumPy arrays, or with
        device_arrays=True of torch tensors on the context's device, written there by the kernels."""
        i = self.info()
        ne, nc = int(i.n_edge), int(i.n_center)
        summary = capi.StrainSummary()
        if not device_arrays:
            out = (np.empty(ne, np.float64), np.empty(3 * nc, np.float64), np.empty(nc, np.float64))
            capi.check(self.lib.avs_get_strain_rates(self.h, int(which), *[a.ctypes.data for a in out], C.byref(summary), capi.MEM_HOST))
            return StrainRates(*out, _strain_summary(summary))
        import torch
        dev = torch.device("cuda", self.device)
        out = tuple(torch.empty(n, dtype=torch.float64, device=dev) for n in (ne, 3 * nc, nc))
        torch.cuda.current_stream(dev).synchronize()   # (the stream rules of octree_cells)
        capi.check(self.lib.avs_get_strain_rates(self.h, int(which), *[a.data_ptr() for a in out], C.byref(summary), capi.MEM_DEVICE))
        torch.cuda.synchronize(dev)
        return StrainRates(*out, _strain_summary(summary))

    def shear_rate_field(self, which=capi.RATES_OF_SOLUTION, device_array=False):
        """The shear rate sqrt(2 eps:eps) on the simulation grid (avs_get_shear_rate_field), the lattice FIELD_VISCOSITY is given on:
        float32 (nz, ny, nx), 0 where no ACTIVE cell covers a cell.  A NumPy array, or with device_array=True a torch tensor on the
        context's device.  With which=capi.RATES_OF_INITIAL_GUESS it is what a shear-dependent viscosity is evaluated from before the
        solve: build_stencils, build_initial_guess, shear_rate_field, set_field(FIELD_VISCOSITY, data=mu(gamma)), assemble, solve."""
        nx, ny, nz = self.field_res
        if not device_array:
            out = np.empty((nz, ny, nx), np.float32)
            capi.check(self.lib.avs_get_shear_rate_field(self.h, int(which), out.ctypes.data, capi.MEM_HOST))
            return out
        import torch
        dev = torch.device("cuda", self.device)
        out = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        capi.check(self.lib.avs_get_shear_rate_field(self.h, int(which), out.data_ptr(), capi.MEM_DEVICE))
        torch.cuda.synchronize(dev)
        return out

    def apply_viscosity_model(self, model, which=capi.RATES_OF_SOLUTION, install=False, device_array=False):
        """A shear-dependent viscosity evaluated on the device (avs_apply_viscosity_model): model is a capi.ViscosityModel (carreau_yasuda /
        herschel_bulkley of this module build one).  Returns (field, summary): the relaxed viscosity on the simulation grid, float32
        (nz, ny, nx) -- covered cells the model of their cell's shear rate, the one-cell fringe around them the mean of its covered
        neighbours, every other cell its current viscosity -- as a NumPy array or, with device_array=True, a torch tensor on the context's
        device, and the ViscositySummary (max_relative_change: the stopping measure of a fixed-point loop).  install=True makes the field
        the context's FIELD_VISCOSITY on the device, as set_field with it would: stencils, system and solution are gone afterwards."""
        nx, ny, nz = self.field_res
        summary = capi.ViscositySummary()
        if not device_array:
            out = np.empty((nz, ny, nx), np.float32)
            capi.check(self.lib.avs_apply_viscosity_model(self.h, int(which), C.byref(model), out.ctypes.data, int(bool(install)), C.byref(summary),
                                                          capi.MEM_HOST))
            return out, _viscosity_summary(summary)
        import torch
        dev = torch.device("cuda", self.device)
        out = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()   # (the stream rules of octree_cells)
        capi.check(self.lib.avs_apply_viscosity_model(self.h, int(which), C.byref(model), out.data_ptr(), int(bool(install)), C.byref(summary),
                                                      capi.MEM_DEVICE))
        torch.cuda.synchronize(dev)
        return out, _viscosity_summary(summary)

    def solve_shear_dependent(self, model, tol=1e-3, max_iters=2500, picard_tol=1e-3, max_picard=20):
        """The fixed-point (Picard) loop of a shear-dependent viscosity, with every field on the device.  The provisional fields are set;
        the model is evaluated on the restricted input velocity and installed; then assemble, solve, evaluate on the solution into a
        device array WITHOUT installing it; max_relative_change <= picard_tol (over covered cells, relaxation included) ends the loop,
        else that array becomes the viscosity and the loop goes again, at most max_picard solves.  On return the context is solved by
        the system that produced its solution (the transfer entries and check_solution work); the viscosity field is the one that
        system was assembled with.  Returns a ShearDependentSolve."""
        self.build_stencils()
        self.build_initial_guess()
        _, initial = self.apply_viscosity_model(model, capi.RATES_OF_INITIAL_GUESS, install=True, device_array=True)
        solves, summaries, converged = [], [], False
        for _ in range(max(1, int(max_picard))):
            self.assemble()
            solves.append(self.solve(tol, max_iters))
            field, summary = self.apply_viscosity_model(model, capi.RATES_OF_SOLUTION, install=False, device_array=True)
            summaries.append(summary)
            if summary.max_relative_change <= picard_tol:
                converged = True
                break
            if len(solves) < max(1, int(max_picard)):
                self.set_field(capi.FIELD_VISCOSITY, 0, field)
        return ShearDependentSolve(converged, initial, tuple(solves), tuple(summaries))

    def edge_stencils(self):
        ne = self.info().n_edge
        return self._stencils(self.lib.avs_get_edge_stencils, ne, ne, capi.EDGE_STENCIL_CAP, capi.EDGE_BOUNDARY_CAP)

    def center_stencils(self):
        nc = self.info().n_center
        return self._stencils(self.lib.avs_get_center_stencils, 3 * nc, nc, capi.CENTER_STENCIL_CAP,
                              capi.CENTER_BOUNDARY_CAP)


@dataclass(frozen=True)
class OctreeCheck:
    """report of check_octree: passed; violations[rule] = lattice entries (rule 7: ids) that break rule `rule` (capi.RULE_*); first =
    (rule, level, axis, i, j, k) of the violating entry that comes first in that order, None when passed"""
    passed: bool
    violations: tuple
    first: tuple | None

    def __bool__(self):
        return self.passed


def _check_octree(fn, handle, what):
    """shared by ViscositySolve.check_octree and DevicePrepass.check_octree"""
    rep = capi.OctreeCheck()
    capi.check(fn(handle, int(what), C.byref(rep)))
    first = None if rep.passed else (rep.first_rule, rep.first_level, rep.first_axis, *rep.first_ijk)
    return OctreeCheck(bool(rep.passed), tuple(int(v) for v in rep.violations), first)


@dataclass(frozen=True)
class StressCheck:
    """report of check_stress_indices: passed; violations[rule] = lattice entries (rules 3 and 8: ids) that break rule `rule`
    (capi.STRESS_RULE_*); first = (rule, level, axis, i, j, k) of the violating entry that comes first in that order, None when passed;
    active_edges / active_centers = entries that carry an id (0 for a kind that was not asked for)"""
    passed: bool
    violations: tuple
    first: tuple | None
    active_edges: int
    active_centers: int

    def __bool__(self):
        return self.passed


def _check_stress_indices(fn, handle, what):
    """shared by ViscositySolve.check_stress_indices and DevicePrepass.check_stress_indices"""
    rep = capi.StressCheck()
    capi.check(fn(handle, int(what), C.byref(rep)))
    first = None if rep.passed else (rep.first_rule, rep.first_level, rep.first_axis, *rep.first_ijk)
    return StressCheck(bool(rep.passed), tuple(int(v) for v in rep.violations), first, int(rep.active_edges), int(rep.active_centers))


@dataclass(frozen=True)
class StrainSummary:
    """avs_strain_summary: n_edge / n_center stencils evaluated; empty_* (cnt == 0) and boundary_* (bcnt > 0) stencils; nonfinite rates;
    edge_lookups[capi.EDGE_LOOKUP_*] = how the cell pass resolved its 12 n_center edge slots; empty_pairs = (cell, edge axis) without an
    edge; dissipation_edge = sum w_e eps_e^2, dissipation_center = sum w_c (exx^2 + eyy^2 + ezz^2); maxima over finite values"""
    which: int
    n_edge: int
    n_center: int
    empty_edges: int
    empty_centers: int
    boundary_edges: int
    boundary_centers: int
    nonfinite: int
    edge_lookups: tuple
    empty_pairs: int
    dissipation_edge: float
    dissipation_center: float
    max_abs_edge_rate: float
    max_abs_center_rate: float
    max_shear_rate: float


@dataclass(frozen=True)
class StrainRates:
    """result of ViscositySolve.strain_rates: edge (n_edge,), center (3 n_center,), cell (n_center,) float64 and the StrainSummary"""
    edge: object
    center: object
    cell: object
    summary: StrainSummary


def _strain_summary(s):
    return StrainSummary(int(s.which), int(s.n_edge), int(s.n_center), int(s.empty_edges), int(s.empty_centers), int(s.boundary_edges),
                         int(s.boundary_centers), int(s.nonfinite), tuple(int(v) for v in s.edge_lookups), int(s.empty_pairs),
                         float(s.dissipation_edge), float(s.dissipation_center), float(s.max_abs_edge_rate), float(s.max_abs_center_rate),
                         float(s.max_shear_rate))


@dataclass(frozen=True)
class ViscositySummary:
    """avs_viscosity_summary: kind of the model, installed; covered / fringe / untouched cells of the simulation grid; clamped_low /
    clamped_high / nonfinite centre ids of n_center; min_viscosity, max_viscosity, max_shear_rate and max_relative_change
    (max |new - old| / old) over covered cells"""
    which: int
    kind: int
    installed: bool
    n_center: int
    covered: int
    fringe: int
    untouched: int
    clamped_low: int
    clamped_high: int
    nonfinite: int
    min_viscosity: float
    max_viscosity: float
    max_shear_rate: float
    max_relative_change: float


def _viscosity_summary(s):
    return ViscositySummary(int(s.which), int(s.kind), bool(s.installed), int(s.n_center), int(s.covered), int(s.fringe), int(s.untouched),
                            int(s.clamped_low), int(s.clamped_high), int(s.nonfinite), float(s.min_viscosity), float(s.max_viscosity),
                            float(s.max_shear_rate), float(s.max_relative_change))


@dataclass(frozen=True)
class ShearDependentSolve:
    """result of ViscositySolve.solve_shear_dependent: converged (the last max_relative_change <= picard_tol); initial = the summary of the
    evaluation on the restricted input velocity; solves[k] the avs_solve_info of solve k and summaries[k] the ViscositySummary of the
    evaluation on its solution"""
    converged: bool
    initial: ViscositySummary
    solves: tuple
    summaries: tuple


def carreau_yasuda(mu_0, mu_inf, lambda_, a, n, mu_min, mu_max, relaxation=1.0):
    """capi.ViscosityModel: mu = mu_inf + (mu_0 - mu_inf) (1 + (lambda gamma)^a)^((n - 1) / a), clamped to [mu_min, mu_max]"""
    return capi.ViscosityModel(kind=capi.VISCOSITY_CARREAU_YASUDA, mu_0=mu_0, mu_inf=mu_inf, lambda_=lambda_, a=a, n=n, mu_min=mu_min,
                               mu_max=mu_max, relaxation=relaxation)


def herschel_bulkley(consistency, n, tau_y, regularisation, mu_min, mu_max, relaxation=1.0):
    """capi.ViscosityModel: mu = consistency gamma^(n - 1) + tau_y (1 - exp(-regularisation gamma)) / gamma (Papanastasiou), clamped"""
    return capi.ViscosityModel(kind=capi.VISCOSITY_HERSCHEL_BULKLEY, consistency=consistency, n=n, tau_y=tau_y, regularisation=regularisation,
                               mu_min=mu_min, mu_max=mu_max, relaxation=relaxation)


def _octree_cells(fn, handle, origin, device_arrays, device):
    """count query, allocate, fill -- shared by ViscositySolve.octree_cells and DevicePrepass.octree_cells"""
    org = None if origin is None else np.ascontiguousarray(origin, np.float64).reshape(3)
    po = None if org is None else org.ctypes.data
    n = C.c_int64()
    per_level = np.zeros(capi.MAX_LEVELS, np.int64)
    capi.check(fn(handle, po, 0, None, None, None, None, C.byref(n), per_level.ctypes.data, capi.MEM_HOST))
    n = int(n.value)
    got = C.c_int64()
    if not device_arrays:
        out = (np.empty((n, 3), np.float32), np.empty(n, np.float32), np.empty(n, np.int32), np.empty((n, 3), np.int32))
        if n:
            capi.check(fn(handle, po, n, *[a.ctypes.data for a in out], C.byref(got), None, capi.MEM_HOST))
        return (*out, per_level)
    import torch
    dev = torch.device("cuda", int(device))
    out = (torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
           torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 3), dtype=torch.int32, device=dev))
    if n:
        # the library writes on the object's stream: it must not start before torch's current stream is done with the memory the
        # caching allocator has just handed out (as sample_velocity does) ...
        torch.cuda.current_stream(dev).synchronize()
        capi.check(fn(handle, po, n, *[a.data_ptr() for a in out], C.byref(got), None, capi.MEM_DEVICE))
        # ... and the records are complete in order of the object's stream only (a stream the library may have created itself, which
        # torch cannot name): torch's streams may read them once the device has drained
        torch.cuda.synchronize(dev)
    return (*out, per_level)


def pcg_csr(row_ptr, col, val, b, x0, tol=1e-3, max_iters=2500, device=0):
    """Seam A (avs_pcg_csr) on host numpy arrays."""
    lib = capi.load()
    rp = np.ascontiguousarray(row_ptr, np.int32)
    cl = np.ascontiguousarray(col, np.int32)
    vl = np.ascontiguousarray(val, np.float64)
    bb = np.ascontiguousarray(b, np.float64)
    x = np.array(x0, np.float64, copy=True)
    info = capi.SolveInfo()
    capi.check(lib.avs_pcg_csr(len(bb), rp.ctypes.data, cl.ctypes.data, vl.ctypes.data, bb.ctypes.data,
                               x.ctypes.data, float(tol), int(max_iters), capi.MEM_HOST, device, None,
                               C.byref(info)))
    return x, info


@dataclass(frozen=True)
class CsrCheck:
    """report of check_csr / check_system: passed; evaluated = bit r: rule r (capi.CSR_RULE_*) was evaluated; violations[rule] = positions
    that break the rule; first = (rule, index, row, col) of the violating position that comes first by (rule, index), None when passed;
    empty_rows, longest_row; with capi.CSR_CHECK_SYMMETRY asymmetric_entries, max_abs_value and max_abs_asymmetry (0 otherwise)"""
    passed: bool
    evaluated: int
    violations: tuple
    first: tuple | None
    empty_rows: int
    longest_row: int
    asymmetric_entries: int
    max_abs_value: float
    max_abs_asymmetry: float

    def __bool__(self):
        return self.passed


def _csr_check(rep):
    first = None if rep.passed else (rep.first_rule, rep.first_index, rep.first_row, rep.first_col)
    return CsrCheck(bool(rep.passed), int(rep.evaluated), tuple(int(v) for v in rep.violations), first, int(rep.empty_rows),
                    int(rep.longest_row), int(rep.asymmetric_entries), float(rep.max_abs_value), float(rep.max_abs_asymmetry))


def check_csr(row_ptr, col, val, b=None, x=None, what=capi.CSR_CHECK_ALL, symmetry_tolerance=0.0, device=0):
    """Is this CSR system one pcg_csr is defined for?  (avs_check_csr on host numpy arrays: eight rules evaluated on the device, see
    include/avs.h.)  A caller checks once when wiring up seam A, not per solve.  Returns a CsrCheck."""
    lib = capi.load()
    rp = np.ascontiguousarray(row_ptr, np.int32)
    cl = np.ascontiguousarray(col, np.int32)
    vl = np.ascontiguousarray(val, np.float64)
    bb = None if b is None else np.ascontiguousarray(b, np.float64)
    xx = None if x is None else np.ascontiguousarray(x, np.float64)
    n = len(rp) - 1
    for name, v in (("b", bb), ("x", xx)):
        if v is not None and len(v) != n:
            raise ValueError(f"{name} has {len(v)} entries for {n} rows")
    if len(cl) != len(vl):
        raise ValueError(f"col has {len(cl)} entries, val {len(vl)}")
    rep = capi.CsrCheck()
    capi.check(lib.avs_check_csr(n, len(cl), rp.ctypes.data, cl.ctypes.data if len(cl) else None, vl.ctypes.data if len(vl) else None,
                                 None if bb is None else bb.ctypes.data, None if xx is None else xx.ctypes.data, int(what),
                                 float(symmetry_tolerance), capi.MEM_HOST, device, None, C.byref(rep)))
    return _csr_check(rep)


@dataclass(frozen=True)
class SolutionCheck:
    """report of check_solution / check_csr_solution (avs_solution_check, include/avs.h): relative_residual = sqrt(residual_norm2 /
    rhs_norm2) of the true r = b - A x over the rows_summed rows whose x_i, b_i and r_i are finite; claimed_error / claimed_converged /
    claimed_iterations: what the solve that left x said of it (NaN / -1 when unknown); evaluated False: seam A found the row pointers or
    columns out of range and walked nothing; residual: every r_i when it was asked for, else None"""
    which: int
    evaluated: bool
    claimed_converged: int
    claimed_iterations: int
    claimed_error: float
    n: int
    nnz: int
    nonfinite_x: int
    nonfinite_b: int
    nonfinite_residual: int
    rows_summed: int
    rhs_norm2: float
    residual_norm2: float
    relative_residual: float
    max_abs_residual: float
    max_residual_row: int
    max_abs_x: float
    x_dot_ax: float
    x_dot_b: float
    update_norm2: float
    max_abs_update: float
    residual: object = None

    @property
    def energy(self):
        """0.5 x.Ax - x.b over the summed rows"""
        return 0.5 * self.x_dot_ax - self.x_dot_b


_SOLUTION_CHECK_FIELDS = [f for f in SolutionCheck.__dataclass_fields__ if f != "residual"]


def _solution_check(rep, residual):
    kinds = SolutionCheck.__annotations__
    return SolutionCheck(**{f: {"int": int, "bool": bool, "float": float}[kinds[f]](getattr(rep, f)) for f in _SOLUTION_CHECK_FIELDS},
                         residual=residual)


def check_csr_solution(row_ptr, col, val, b, x, x0=None, residual=False, device=0):
    """Did x solve this CSR system?  (avs_check_csr_solution on host numpy arrays: the true residual b - A x in fp64, rows added in stored
    order; rules 0 and 1 of check_csr run first, and .evaluated is False if they fail.)  x0: the initial guess, for the update figures.
    Returns a SolutionCheck, with residual=True its .residual filled."""
    lib = capi.load()
    rp = np.ascontiguousarray(row_ptr, np.int32)
    cl = np.ascontiguousarray(col, np.int32)
    vl = np.ascontiguousarray(val, np.float64)
    n = len(rp) - 1
    vecs = {k: None if v is None else np.ascontiguousarray(v, np.float64) for k, v in (("b", b), ("x", x), ("x0", x0))}
    for name, v in vecs.items():
        if v is not None and len(v) != n:
            raise ValueError(f"{name} has {len(v)} entries for {n} rows")
    if len(cl) != len(vl):
        raise ValueError(f"col has {len(cl)} entries, val {len(vl)}")
    out = np.empty(n, np.float64) if residual else None
    ptr = lambda a: None if a is None or len(a) == 0 else a.ctypes.data
    rep = capi.SolutionCheck()
    capi.check(lib.avs_check_csr_solution(n, len(cl), rp.ctypes.data, ptr(cl), ptr(vl), ptr(vecs["b"]), ptr(vecs["x"]), ptr(vecs["x0"]),
                                          ptr(out), capi.MEM_HOST, device, None, C.byref(rep)))
    return _solution_check(rep, out)


@dataclass(frozen=True)
class Spectrum:
    """report of estimate_spectrum / estimate_csr_spectrum (avs_spectrum, include/avs.h): the extreme Ritz values of steps_taken Lanczos
    steps on the operator the solve inverts, each with the distance within which an eigenvalue lies (lambda_*_bound); condition_estimate =
    lambda_max / lambda_min is a LOWER bound of the condition number, iteration_bound the classical CG bound for `tolerance` (-1: none);
    indefinite: a Ritz value <= 0, the matrix is not positive definite; evaluated False: the row pointers or columns are out of range
    (seam A) or bad_diagonal rows have no positive finite diagonal.  alpha, beta, ritz: NumPy arrays (steps, steps + 1, steps entries; 0
    behind what steps_taken wrote); scale, basis: as asked for, else None"""
    evaluated: bool
    op: int
    start: int
    steps_asked: int
    steps_taken: int
    breakdown: bool
    nonfinite: bool
    indefinite: bool
    n: int
    nnz: int
    bad_diagonal: int
    start_norm: float
    lambda_min: float
    lambda_max: float
    lambda_min_bound: float
    lambda_max_bound: float
    gershgorin_max: float
    condition_estimate: float
    tolerance: float
    iteration_bound: int
    alpha: object = None
    beta: object = None
    ritz: object = None
    scale: object = None
    basis: object = None


_SPECTRUM_ARRAYS = ("alpha", "beta", "ritz", "scale", "basis")
_SPECTRUM_FIELDS = [f for f in Spectrum.__dataclass_fields__ if f not in _SPECTRUM_ARRAYS]


def _estimate(call, n, op, start, steps, tolerance, scale, basis, device):
    """call(op, start, steps, tolerance, alpha, beta, ritz, scale, basis, where, report) -> status; device: None for NumPy outputs"""
    steps = int(steps)
    room = max(steps, 0)
    alpha, beta, ritz = np.zeros(room), np.zeros(room + 1), np.zeros(room)
    s_out = b_out = None
    if device is None:
        s_out = np.zeros(n) if scale else None
        b_out = np.zeros((room + 1, n)) if basis else None
        ptr = lambda a: None if a is None else a.ctypes.data
    else:
        import torch
        dev = torch.device("cuda", device)
        s_out = torch.zeros(n, dtype=torch.float64, device=dev) if scale else None
        b_out = torch.zeros((room + 1, n), dtype=torch.float64, device=dev) if basis else None
        torch.cuda.current_stream(dev).synchronize()   # (the stream rules of octree_cells)
        ptr = lambda a: None if a is None else a.data_ptr()
    rep = capi.Spectrum()
    capi.check(call(int(op), int(start), steps, float(tolerance), alpha.ctypes.data, beta.ctypes.data, ritz.ctypes.data, ptr(s_out), ptr(b_out),
                    capi.MEM_HOST if device is None else capi.MEM_DEVICE, C.byref(rep)))
    if device is not None:
        import torch
        torch.cuda.synchronize(torch.device("cuda", device))
    kinds = Spectrum.__annotations__
    return Spectrum(**{f: {"int": int, "bool": bool, "float": float}[kinds[f]](getattr(rep, f)) for f in _SPECTRUM_FIELDS},
                    alpha=alpha, beta=beta, ritz=ritz, scale=s_out, basis=b_out)


def estimate_csr_spectrum(row_ptr, col, val, b=None, x0=None, start_vector=None, op=capi.SPECTRUM_OF_JACOBI, start=None, steps=32, tolerance=1e-3,
                          scale=False, basis=False, device=0):
    """The spectrum of this CSR matrix as a CG solve sees it (avs_estimate_csr_spectrum on host numpy arrays: `steps` Lanczos steps in fp64
    on D^-1/2 A D^-1/2, or on A with op=capi.SPECTRUM_OF_MATRIX; rules 0 and 1 of check_csr run first, and .evaluated is False if they
    fail).  start: capi.SPECTRUM_START_*; None picks the caller's start_vector if given, the scaled residual of (b, x0) if both are given,
    else the hash vector.  Returns a Spectrum, with scale=True / basis=True its .scale / .basis filled."""
    lib = capi.load()
    rp = np.ascontiguousarray(row_ptr, np.int32)
    cl = np.ascontiguousarray(col, np.int32)
    vl = np.ascontiguousarray(val, np.float64)
    n = len(rp) - 1
    vecs = {k: None if v is None else np.ascontiguousarray(v, np.float64) for k, v in (("b", b), ("x0", x0), ("start_vector", start_vector))}
    for name, v in vecs.items():
        if v is not None and len(v) != n:
            raise ValueError(f"{name} has {len(v)} entries for {n} rows")
    if len(cl) != len(vl):
        raise ValueError(f"col has {len(cl)} entries, val {len(vl)}")
    if start is None:
        start = capi.SPECTRUM_START_VECTOR if start_vector is not None else \
            capi.SPECTRUM_START_RESIDUAL if b is not None and x0 is not None else capi.SPECTRUM_START_HASH
    ptr = lambda a: None if a is None or len(a) == 0 else a.ctypes.data
    return _estimate(lambda op_, start_, steps_, tol, *outs: lib.avs_estimate_csr_spectrum(
        n, len(cl), rp.ctypes.data, ptr(cl), ptr(vl), ptr(vecs["b"]), ptr(vecs["x0"]), ptr(vecs["start_vector"]), op_, start_, steps_, tol, *outs[:6],
        device, None, outs[6]), n, op, start, steps, tolerance, scale, basis, None)


class DevicePrepass:
    """Pre-pass on the GPU (avs_prepass_*): liquid / solid SDF -> weights, label pyramid, index pyramids."""

    def __init__(self, res, dx, levels, n_super=3, extrapolation=0.5, device=0, stream=None, field_res=None, probe=False):
        """`res`: octree (power-of-two) resolution; `field_res`: the simulation grid the SDFs live on when it is smaller
        (HDK_OctreeGrid::init pads to powers of two, oct.cpp:10-24); None = res.  probe=True: the object lives in libavs_probe.so, for a
        ViscositySolve(probe=True) to apply it to -- the two must come from the same library."""
        self.lib = capi.load(probe=probe)
        self.res = tuple(int(r) for r in res)
        fr = tuple(int(r) for r in field_res) if field_res is not None else (0, 0, 0)
        self.field_res = tuple(fr[a] or self.res[a] for a in range(3))
        d = capi.PrepassDesc(self.res[0], self.res[1], self.res[2], float(dx), int(levels), int(n_super),
                             float(extrapolation), int(device), C.c_void_p(stream or 0), fr[0], fr[1], fr[2])
        h = C.c_void_p()
        capi.check(self.lib.avs_prepass_create(C.byref(d), C.byref(h)))
        self.h = h
        self.device = int(device)
        self.info = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.avs_prepass_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, liquid, solid=None):
        pl, wl = capi.ptr_of(liquid)
        ps, ws = capi.ptr_of(solid)
        if solid is not None and ws != wl:
            raise ValueError("liquid and solid must live in the same memory space")
        capi.check(self.lib.avs_prepass_run(self.h, pl, ps, wl))
        info = capi.PrepassInfo()
        capi.check(self.lib.avs_prepass_get_info(self.h, C.byref(info)))
        self.info = info
        return info

    def set_slab(self, cut_axis, cuts, rank, allreduce):
        """Slab-local mode with the caller's own all-reduce (a hosted group): allreduce(device_pointer, count, stream) sums `count` int32
        in place over all ranks and returns when the result is there.  cuts None: off."""
        if cuts is None:
            self._slab_cb = None
            capi.check(self.lib.avs_prepass_set_slab(self.h, 0, None, 1, 0, capi.ALLREDUCE_I32_FN(0), None))
            return

        def cb(ptr, count, stream, user):
            try:
                allreduce(ptr, count, stream)
                return 0
            except Exception:  # pragma: no cover
                return capi.EINTERNAL if hasattr(capi, "EINTERNAL") else 7
        self._slab_cb = capi.ALLREDUCE_I32_FN(cb)   # (kept alive with the object)
        c = np.ascontiguousarray(cuts, np.int32)
        capi.check(self.lib.avs_prepass_set_slab(self.h, int(cut_axis), c.ctypes.data, len(c) - 1, int(rank), self._slab_cb, None))

    def window(self):
        """(lo[levels], hi[levels], (n_velocity, n_edge, n_center) inside the window) of the last run."""
        lo = np.zeros(8, np.int32)
        hi = np.zeros(8, np.int32)
        nw = np.zeros(3, np.int64)
        capi.check(self.lib.avs_prepass_get_window(self.h, lo.ctypes.data, hi.ctypes.data, nw.ctypes.data))
        L = self.info.levels if self.info is not None else 8
        return lo[:L], hi[:L], tuple(int(v) for v in nw)

    def set_option(self, option, value):
        """avs_prepass_set_option: capi.PREPASS_OPTION_FINE_BANDWIDTH -- the reference's "Fine Layer Bandwidth" (cells within
        dx * max(2, value) inside the surface stay fine); capi.PREPASS_OPTION_APPLY_SOLID_WEIGHTS -- its "Apply Solid Weights" (0 / 1:
        centre and edge weights divided by the open-space fraction of the solid SDF given to run()); takes effect at the next run."""
        capi.check(self.lib.avs_prepass_set_option(self.h, int(option), float(value)))

    def set_refinement(self, field=None, threshold=0.0, dilate=0):
        """avs_prepass_set_refinement: the cells of `field` (simulation grid, float32, numpy array or torch tensor, host or device --
        ViscositySolve.shear_rate_field(device_array=True) plugs in) above `threshold`, dilated by `dilate` cells, stay fine in every
        following run wherever the surface rule would coarsen them.  field None: no refinement."""
        if field is None:
            capi.check(self.lib.avs_prepass_set_refinement(self.h, None, 0.0, 0, capi.MEM_HOST))
            return
        if isinstance(field, np.ndarray):
            field = np.ascontiguousarray(field, np.float32)
        else:
            import torch
            if field.dtype != torch.float32:
                raise ValueError("the indicator must be float32")
            field = field.contiguous()
            if field.is_cuda:   # (the library reads it on the pre-pass's stream)
                torch.cuda.current_stream(field.device).synchronize()
        n = self.field_res[0] * self.field_res[1] * self.field_res[2]
        if int(field.size if isinstance(field, np.ndarray) else field.numel()) != n:
            raise ValueError(f"the indicator must have the {self.field_res} cells of the simulation grid")
        ptr, where = capi.ptr_of(field)
        capi.check(self.lib.avs_prepass_set_refinement(self.h, ptr, float(threshold), int(dilate), where))

    def refinement(self):
        """The refinement flags (0 / 1) on the octree centre lattice, shaped like mask()."""
        out = np.empty(self._shape(2, 0, 0), np.int8)
        capi.check(self.lib.avs_prepass_get_refinement(self.h, out.ctypes.data, capi.MEM_HOST))
        return out

    def refinement_info(self):
        """avs_refinement_info: threshold, dilate_cells, active, the set call's seeds / flagged counts and time, the last run's refined"""
        info = capi.RefinementInfo()
        info.struct_size = C.sizeof(capi.RefinementInfo)
        capi.check(self.lib.avs_prepass_get_refinement_info(self.h, C.byref(info)))
        return info

    def solid_weights_info(self):
        """avs_solid_weights_info: enabled, applied, extrapolation, and per lattice (centre, edge x, y, z) the last run's modified /
        zeroed / above_one counts and max_weight; near_bricks"""
        info = capi.SolidWeightsInfo()
        info.struct_size = C.sizeof(capi.SolidWeightsInfo)
        capi.check(self.lib.avs_prepass_get_solid_weights_info(self.h, C.byref(info)))
        return info

    def apply(self, solver):
        capi.check(self.lib.avs_prepass_apply(self.h, solver.h))
        solver.counts = (self.info.n_velocity, self.info.n_edge, self.info.n_center)

    def octree_cells(self, origin=None, device_arrays=False):
        """The ACTIVE cells of the last run's label pyramid as points (avs_prepass_get_octree_cells): what ViscositySolve.octree_cells
        returns, without a solve context ("Only Output Octree")."""
        return _octree_cells(self.lib.avs_prepass_get_octree_cells, self.h, origin, device_arrays, self.device)

    def check_octree(self, what=capi.CHECK_LABELS | capi.CHECK_VELOCITY_INDICES):
        """The invariants of the last run's label and velocity index pyramids (avs_prepass_check_octree): what
        ViscositySolve.check_octree returns, without a solve context."""
        return _check_octree(self.lib.avs_prepass_check_octree, self.h, what)

    def check_stress_indices(self, what=capi.CHECK_EDGE_INDICES | capi.CHECK_CENTER_INDICES):
        """The invariants of the last run's edge and centre stress index pyramids (avs_prepass_check_stress_indices): what
        ViscositySolve.check_stress_indices returns, without a solve context."""
        return _check_stress_indices(self.lib.avs_prepass_check_stress_indices, self.h, what)

    def _shape(self, kind, level, axis):
        r = [self.res[0] >> level, self.res[1] >> level, self.res[2] >> level]
        if kind == 0:
            r[axis] += 1
        elif kind == 1:
            r = [r[a] + (a != axis) for a in range(3)]
        return (r[2], r[1], r[0])

    def labels(self, level):
        out = np.empty(self._shape(2, level, 0), np.int8)
        capi.check(self.lib.avs_prepass_get_labels(self.h, level, out.ctypes.data, capi.MEM_HOST))
        return out

    def mask(self):
        out = np.empty(self._shape(2, 0, 0), np.int8)
        capi.check(self.lib.avs_prepass_get_mask(self.h, out.ctypes.data, capi.MEM_HOST))
        return out

    def index(self, kind, level, axis=0):
        out = np.empty(self._shape(kind, level, axis), np.int32)
        capi.check(self.lib.avs_prepass_get_index(self.h, kind, level, axis, out.ctypes.data, capi.MEM_HOST))
        return out

    def regular_index(self, axis):
        out = np.empty(self._shape(0, 0, axis), np.int32)
        capi.check(self.lib.avs_prepass_get_regular_index(self.h, axis, out.ctypes.data, capi.MEM_HOST))
        return out

    def weights(self, kind, axis=0):
        k = {capi.FIELD_CENTER_WEIGHTS: 2, capi.FIELD_EDGE_WEIGHTS: 1, capi.FIELD_FACE_WEIGHTS: 0}[kind]
        out = np.empty(self._shape(k, 0, axis), np.float32)
        capi.check(self.lib.avs_prepass_get_weights(self.h, kind, axis, out.ctypes.data, capi.MEM_HOST))
        return out
