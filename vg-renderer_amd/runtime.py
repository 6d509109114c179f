"""Python plumbing over the C-ABI (libvgx.so): context, path sets, batch calls on torch device memory.

PyTorch is used only for device allocations and streams; every geometry computation happens in the
HIP kernels behind include/vgx.h. There is NO CPU fallback: if libvgx.so is missing or no gfx950 device is
present, construction raises.
"""
import ctypes as C
import os
import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VGX_LIB", os.path.join(_HERE, "libvgx.so"))  # VGX_LIB: tuning experiments only
_lib = None


class VgxError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        name = lib().vgx_status_string(status).decode() if _lib is not None else str(status)
        super().__init__("%s failed: %s (%d)" % (where, name, status))


def lib():
    """Load libvgx.so (built in-tree by `__graft_entry__.build()` / csrc/Makefile). Fails loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libvgx.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` (HIP extension is mandatory, there is no CPU fallback)")
        # import torch first so that its HIP runtime (same SONAME) is the one both sides use
        import torch  # noqa: F401
        _lib = capi.bind(C.CDLL(LIB_PATH), capi.VGX_SYMBOLS)
    return _lib


def _check(st, where):
    if st != capi.VGX_OK:
        raise VgxError(st, where)


def validate_pathset(ps):
    """Host-only grammar / finiteness validation (no device needed)."""
    d = ps.desc()
    return lib().vgx_pathset_validate(C.byref(d))


class Context:
    def __init__(self, device=0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: vg-renderer_amd has no CPU fallback")
        self.device = device
        self._h = C.c_void_p()
        torch.cuda.set_device(device)
        torch.zeros(1, device="cuda:%d" % device)  # make sure the primary context exists
        _check(lib().vgx_create(device, C.byref(self._h)), "vgx_create")

    def close(self):
        if self._h:
            lib().vgx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def scratch_bytes(self):
        return int(lib().vgx_scratch_bytes(self._h))

    def reserve(self, ndraws, sizes):
        """vgx_reserve: size the scratch for batches up to `sizes` (a dict or capi.Sizes: num_cmd_instances, num_poly_vertices,
        num_subpaths, num_meshes) of `ndraws` draws, so that such a batch takes one tessellate_immediate call."""
        if isinstance(sizes, dict):
            z = capi.Sizes()
            for k in ("num_cmd_instances", "num_poly_vertices", "num_subpaths", "num_meshes"):
                setattr(z, k, int(sizes.get(k, 0)))
            sizes = z
        _check(lib().vgx_reserve(self._h, int(ndraws), C.byref(sizes)), "vgx_reserve")

    def reserve_dashed(self, ndraws, sizes, dash_sizes):
        """vgx_reserve_dashed: size the scratch for frames up to `sizes` (what tessellate_dashed leaves in dev_sizes) whose dashed
        strokes make up to `dash_sizes` (its dev_dash_sizes: num_subpaths pieces of num_poly_vertices vertices), so that such a
        frame takes one tessellate_dashed call. Dicts or capi.Sizes."""
        def as_sizes(d):
            if not isinstance(d, dict):
                return d
            z = capi.Sizes()
            for k in ("num_cmd_instances", "num_poly_vertices", "num_subpaths", "num_meshes"):
                setattr(z, k, int(d.get(k, 0)))
            return z
        sizes, dash_sizes = as_sizes(sizes), as_sizes(dash_sizes)
        _check(lib().vgx_reserve_dashed(self._h, int(ndraws), C.byref(sizes), C.byref(dash_sizes)), "vgx_reserve_dashed")

    def set_profiling(self, on):
        _check(lib().vgx_set_profiling(self._h, 1 if on else 0), "vgx_set_profiling")

    def set_static_batches(self, on):
        """vgx_set_static_batches: batches keep their structure between counts (only transforms / colours move): the whole draw
        list becomes one template at the next tessellate_count, a step is then one kernel; a structural change -> VGX_E_STALE."""
        _check(lib().vgx_set_static_batches(self._h, 1 if on else 0), "vgx_set_static_batches")

    def set_assembly(self, drawcmds=None, max_vb_vertices=0, dev_num=None, split_state=False, uv=None, uv_value=None):
        """Arms draw-command assembly (vgx_set_assembly) with a uint8 device tensor of 48-byte vgx_drawcmd records,
        or disarms it (drawcmds=None). split_state: VGX_ASM_SPLIT_STATE. uv: device tensor of the UV stream (int16 [n,2]
        = 4 bytes per vertex, or float32 [n,2] = 8), uv_value: the white-pixel UV as a tuple of raw uint32 words.
        The tensors must stay alive while armed."""
        if drawcmds is None:
            _check(lib().vgx_set_assembly(self._h, None), "vgx_set_assembly")
            self._asm_keep = None
            return
        a = capi.Assembly()
        a.drawcmds = drawcmds.data_ptr()
        a.cap_drawcmds = drawcmds.numel() // capi.drawcmd_dtype.itemsize
        a.dev_num_drawcmds = dev_num.data_ptr() if dev_num is not None else None
        a.max_vb_vertices = max_vb_vertices
        a.flags = capi.ASM_SPLIT_STATE if split_state else 0
        a.reserved = 0
        if uv is not None:
            a.uv = uv.data_ptr()
            a.uv_bytes = uv.element_size() * 2
            a.uv_value[0] = int(uv_value[0]) & 0xFFFFFFFF
            a.uv_value[1] = int(uv_value[1]) & 0xFFFFFFFF if len(uv_value) > 1 else 0
        _check(lib().vgx_set_assembly(self._h, C.byref(a)), "vgx_set_assembly")
        self._asm_keep = (drawcmds, dev_num, uv)

    def failure_info(self):
        """Device status + why the single-pass kernel gave up, if it did (vgx_get_failure_info; synchronises)."""
        fi = capi.FailureInfo()
        _check(lib().vgx_get_failure_info(self._h, C.byref(fi), _stream_ptr()), "vgx_get_failure_info")
        return fi.as_dict()

    def stage_times(self, ncalls=1):
        """Per-kernel HIP-event times of the last profiled call, or their average over the last `ncalls` calls."""
        st = capi.StageTimes()
        _check(lib().vgx_get_stage_times_avg(self._h, C.byref(st), int(ncalls)), "vgx_get_stage_times_avg")
        return [(st.name[i].decode(), float(st.ms[i])) for i in range(st.num_stages)]


class PathSet:
    """Path definitions resident in HBM (vgx_pathset)."""

    def __init__(self, ctx, arrays):
        self.ctx = ctx
        self.arrays = arrays
        self._h = C.c_void_p()
        d = arrays.desc()
        _check(lib().vgx_pathset_create(ctx.handle, C.byref(d), C.byref(self._h)), "vgx_pathset_create")

    def close(self):
        if self._h and self.ctx.handle:
            lib().vgx_pathset_destroy(self.ctx.handle, self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h


def pin_draws(draws):
    """numpy draw records -> uint8 torch tensor in PINNED host memory: where a caller that cares about the upload writes its draw
    records in the first place (pageable memory reaches the device at 7-20 GB/s through the runtime's staging, pinned at ~55)."""
    import torch
    raw = np.ascontiguousarray(draws).view(np.uint8).reshape(-1)
    t = torch.empty(raw.shape[0], dtype=torch.uint8, pin_memory=True)
    t.numpy()[:] = raw
    return t


def upload_draws(draws, device=0):
    """draw records (numpy, or a pinned uint8 tensor from pin_draws) -> uint8 torch tensor in HBM (64 bytes per draw)."""
    import torch
    if isinstance(draws, torch.Tensor):
        return draws.to("cuda:%d" % device, non_blocking=True)
    raw = np.ascontiguousarray(draws).view(np.uint8).reshape(-1)
    return torch.from_numpy(raw).to("cuda:%d" % device)


def _stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class FlatResult:
    pass


class MeshResult:
    pass


def flatten(ctx, pset, draws_dev, ndraws, apply_transform=False, to_host=True, entry=None):
    """The flatten entry points. draws_dev: uint8 torch tensor from upload_draws.
    entry "two_phase": vgx_flatten_count + vgx_flatten_emit; "one_walk": vgx_flatten into buffers of exactly the counted sizes;
    "both" (default; VGX_FLATTEN_ENTRY overrides): the two-phase result, after checking that vgx_flatten produced the same
    bytes -- polyline, sub-path records, per-draw records, totals -- so that every caller of this helper pins both entry points."""
    import torch
    entry = entry or os.environ.get("VGX_FLATTEN_ENTRY", "both")
    if entry in ("one_walk", "both"):
        r2 = _flatten_two_phase(ctx, pset, draws_dev, ndraws, apply_transform, to_host=False)
        r1 = flatten_one_walk(ctx, pset, draws_dev, ndraws, apply_transform, cap_poly=r2.sizes["num_poly_vertices"], cap_subs=r2.sizes["num_subpaths"], to_host=to_host)
        if entry == "both":
            for k in ("num_poly_vertices", "num_subpaths", "num_meshes", "num_serial_draws", "num_cmd_instances"):
                assert r1.sizes[k] == r2.sizes[k], ("vgx_flatten vs two-phase", k, r1.sizes[k], r2.sizes[k])
            npv, nsp = r2.sizes["num_poly_vertices"], r2.sizes["num_subpaths"]
            assert torch.equal(r1.poly_dev[:npv].view(torch.int32), r2.poly_dev[:npv].view(torch.int32)), "vgx_flatten: polyline differs from the two-phase entry"
            assert torch.equal(r1.subs_dev[:nsp * 16], r2.subs_dev[:nsp * 16]), "vgx_flatten: sub-path records differ from the two-phase entry"
            assert torch.equal(r1.dinfo_dev[:ndraws * 40], r2.dinfo_dev[:ndraws * 40]), "vgx_flatten: per-draw records differ from the two-phase entry"
        return r1
    return _flatten_two_phase(ctx, pset, draws_dev, ndraws, apply_transform, to_host)


def _flatten_two_phase(ctx, pset, draws_dev, ndraws, apply_transform=False, to_host=True):
    import torch
    L = lib()
    sizes = capi.Sizes()
    s = _stream_ptr()
    _check(L.vgx_flatten_count(ctx.handle, pset.handle, draws_dev.data_ptr(), ndraws, C.byref(sizes), s), "vgx_flatten_count")
    dev = draws_dev.device
    npv, nsp = int(sizes.num_poly_vertices), int(sizes.num_subpaths)
    poly = torch.empty((max(npv, 1), 2), dtype=torch.float32, device=dev)
    subs = torch.empty(max(nsp, 1) * 16, dtype=torch.uint8, device=dev)
    dinfo = torch.empty(max(ndraws, 1) * 40, dtype=torch.uint8, device=dev)
    out = capi.FlatOut(poly.data_ptr(), subs.data_ptr(), dinfo.data_ptr(), npv, nsp)
    _check(L.vgx_flatten_emit(ctx.handle, pset.handle, draws_dev.data_ptr(), ndraws, int(apply_transform), C.byref(out), s), "vgx_flatten_emit")
    torch.cuda.synchronize()
    r = FlatResult()
    r.sizes = sizes.as_dict()
    r.poly_dev, r.subs_dev, r.dinfo_dev = poly, subs, dinfo
    if to_host:
        r.poly = poly[:npv].cpu().numpy()
        r.subpaths = subs[:nsp * 16].cpu().numpy().view(capi.subpath_dtype)
        r.draw_info = dinfo[:ndraws * 40].cpu().numpy().view(capi.draw_info_dtype)
    return r


class FlatBuffers:
    """Caller-owned output buffers of vgx_flatten in HBM (vgx_flat_out) + the device-side totals / status words."""

    def __init__(self, device, npoly, nsubs, ndraws):
        import torch
        self.cap = (int(npoly), int(nsubs))
        self.poly = torch.empty((max(int(npoly), 1), 2), dtype=torch.float32, device=device)
        self.subs = torch.empty(max(int(nsubs), 1) * 16, dtype=torch.uint8, device=device)
        self.dinfo = torch.empty(max(int(ndraws), 1) * 40, dtype=torch.uint8, device=device)
        self.dev_sizes = torch.zeros(10, dtype=torch.int64, device=device)
        self.dev_status = torch.zeros(1, dtype=torch.int32, device=device)

    def out_struct(self):
        return capi.FlatOut(self.poly.data_ptr(), self.subs.data_ptr(), self.dinfo.data_ptr(), self.cap[0], self.cap[1])


def flatten_async(ctx, pset, draws_dev, ndraws, bufs, apply_transform=False):
    """vgx_flatten: the ordered one-walk flatten, single asynchronous call; totals / status land in bufs.dev_*."""
    out = bufs.out_struct()
    _check(lib().vgx_flatten(ctx.handle, pset.handle, draws_dev.data_ptr(), ndraws, int(apply_transform), C.byref(out),
                             bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_flatten")


def flatten_one_walk(ctx, pset, draws_dev, ndraws, apply_transform=False, cap_poly=None, cap_subs=None, to_host=True):
    """vgx_flatten into buffers of the given capacities (default: generous), results like `flatten`. Raises VgxError with the
    device status when it is not VGX_OK (the sizes of the failed call stay available as `.sizes` on the exception)."""
    import torch
    dev = draws_dev.device
    if cap_poly is None or cap_subs is None:
        # sizes from the two-phase entry: callers that know their capacities pass them
        z = capi.Sizes()
        _check(lib().vgx_flatten_count(ctx.handle, pset.handle, draws_dev.data_ptr(), ndraws, C.byref(z), _stream_ptr()), "vgx_flatten_count")
        cap_poly = int(z.num_poly_vertices) if cap_poly is None else cap_poly
        cap_subs = int(z.num_subpaths) if cap_subs is None else cap_subs
    bufs = FlatBuffers(dev, cap_poly, cap_subs, ndraws)
    flatten_async(ctx, pset, draws_dev, ndraws, bufs, apply_transform)
    torch.cuda.synchronize()
    st = int(bufs.dev_status.item())
    z = bufs.dev_sizes.cpu().numpy()
    names = [k for k, _ in capi.Sizes._fields_]
    sizes = {k: int(z[i]) for i, k in enumerate(names)}
    if st != capi.VGX_OK:
        e = VgxError(st, "vgx_flatten")
        e.sizes = sizes
        raise e
    r = FlatResult()
    r.sizes = sizes
    r.poly_dev, r.subs_dev, r.dinfo_dev = bufs.poly, bufs.subs, bufs.dinfo
    if to_host:
        npv, nsp = sizes["num_poly_vertices"], sizes["num_subpaths"]
        r.poly = bufs.poly[:npv].cpu().numpy()
        r.subpaths = bufs.subs[:nsp * 16].cpu().numpy().view(capi.subpath_dtype)
        r.draw_info = bufs.dinfo[:ndraws * 40].cpu().numpy().view(capi.draw_info_dtype)
    return r


class MeshBuffers:
    """Caller-owned output buffers in HBM (vgx_mesh_out)."""

    def __init__(self, device, nverts, nidx, nmeshes):
        import torch
        self.cap = (int(nverts), int(nidx), int(nmeshes))
        self.pos = torch.empty((max(nverts, 1), 2), dtype=torch.float32, device=device)
        self.color = torch.empty(max(nverts, 1), dtype=torch.int32, device=device)
        self.idx = torch.empty(max(nidx, 1), dtype=torch.int16, device=device)
        self.meshes = torch.empty(max(nmeshes, 1) * 32, dtype=torch.uint8, device=device)
        self.dev_sizes = torch.zeros(10, dtype=torch.int64, device=device)
        self.dev_status = torch.zeros(1, dtype=torch.int32, device=device)

    def out_struct(self):
        return capi.MeshOut(self.pos.data_ptr(), self.color.data_ptr(), self.idx.data_ptr(), self.meshes.data_ptr(),
                            self.cap[0], self.cap[1], self.cap[2])

    def view(self, v0, nv, i0, ni, m0, nm):
        """A tile of these buffers: vertices [v0, v0 + nv), indices [i0, i0 + ni), mesh records [m0, m0 + nm) as buffers of
        their own (same memory; own totals / status words) -- what one sub-batch of a frame is tessellated into."""
        import torch
        t = MeshBuffers.__new__(MeshBuffers)
        t.cap = (int(nv), int(ni), int(nm))
        t.pos = self.pos[v0:v0 + max(nv, 1)]
        t.color = self.color[v0:v0 + max(nv, 1)]
        t.idx = self.idx[i0:i0 + max(ni, 1)]
        t.meshes = self.meshes[m0 * 32:(m0 + max(nm, 1)) * 32]
        t.dev_sizes = torch.zeros(10, dtype=torch.int64, device=self.pos.device)
        t.dev_status = torch.zeros(1, dtype=torch.int32, device=self.pos.device)
        return t


def partition(ctx, pset, draws_dev, ndraws, nparts):
    """vgx_partition: contiguous draw ranges of about equal predicted output. Returns (bounds [nparts + 1], weights [nparts])."""
    bounds = (C.c_uint64 * (nparts + 1))()
    weights = (C.c_uint64 * nparts)()
    _check(lib().vgx_partition(ctx.handle, pset.handle, draws_dev.data_ptr(), ndraws, nparts, bounds, weights, _stream_ptr()), "vgx_partition")
    return list(bounds), list(weights)


def tessellate_count(ctx, pset, draws_dev, ndraws):
    sizes = capi.Sizes()
    _check(lib().vgx_tessellate_count(ctx.handle, pset.handle, draws_dev.data_ptr(), ndraws, C.byref(sizes), _stream_ptr()), "vgx_tessellate_count")
    return sizes.as_dict()


def tessellate_emit(ctx, pset, draws_dev, ndraws, bufs):
    out = bufs.out_struct()
    _check(lib().vgx_tessellate_emit(ctx.handle, pset.handle, draws_dev.data_ptr(), ndraws, C.byref(out), _stream_ptr()), "vgx_tessellate_emit")


def tessellate_async(ctx, pset, draws_dev, ndraws, bufs):
    """Steady-state call: whole pipeline, no host round trip; totals/status land in bufs.dev_*."""
    out = bufs.out_struct()
    _check(lib().vgx_tessellate(ctx.handle, pset.handle, draws_dev.data_ptr(), ndraws, C.byref(out),
                                bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_tessellate")


def tessellate_immediate(ctx, pset, draws_dev, ndraws, bufs):
    """vgx_tessellate_immediate: a batch the context need never have counted, asynchronous like tessellate_async. The verdict
    lands in bufs.dev_status (VGX_OK / VGX_E_NOSPACE: grow the buffers to bufs.dev_sizes / VGX_E_GROWN: call again), the
    totals in bufs.dev_sizes."""
    out = bufs.out_struct()
    _check(lib().vgx_tessellate_immediate(ctx.handle, pset.handle, draws_dev.data_ptr(), ndraws, C.byref(out),
                                          bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_tessellate_immediate")


class ImmediateResult:
    """What tessellate_grow ends with: the status of every call (the last one VGX_OK) and the batch's totals."""

    def __init__(self, statuses, sizes):
        self.statuses = statuses
        self.sizes = sizes

    @property
    def calls(self):
        return len(self.statuses)


def _grown(cap, need, growth):
    return cap if need <= cap else max(int(need), int(cap * growth))


def tessellate_grow(ctx, pset, draws_dev, ndraws, bufs=None, growth=1.5, max_calls=3):
    """The immediate-mode loop: tessellate_immediate until VGX_OK. After VGX_E_NOSPACE the buffers grow to the totals in
    dev_sizes, by at least `growth` times (as the reference's allocIndices / allocVertices grow theirs, src/vg.cpp:5321-5357);
    after VGX_E_GROWN the context grows its own scratch at the next call. Synchronises the stream once per call (to read the
    verdict). Returns (ImmediateResult, buffers) -- the buffers may be new ones."""
    if bufs is None:
        bufs = MeshBuffers(draws_dev.device, 1024, 1024, 64)
    statuses = []
    for _ in range(max_calls):
        tessellate_immediate(ctx, pset, draws_dev, ndraws, bufs)
        st = int(bufs.dev_status.item())  # (synchronises)
        statuses.append(st)
        sizes = capi.Sizes.from_buffer_copy(bufs.dev_sizes.cpu().numpy().tobytes()).as_dict()
        if st == capi.VGX_OK:
            return ImmediateResult(statuses, sizes), bufs
        if st == capi.VGX_E_NOSPACE:
            nv, ni, nm = bufs.cap
            bufs = MeshBuffers(draws_dev.device, _grown(nv, sizes["num_vertices"], growth), _grown(ni, sizes["num_indices"], growth),
                               _grown(nm, sizes["num_meshes"], growth))
        elif st != capi.VGX_E_GROWN:
            raise VgxError(st, "vgx_tessellate_immediate (device)")
    raise VgxError(statuses[-1], "tessellate_grow: no VGX_OK within %d calls (%s)" % (max_calls, statuses))


def tessellate(ctx, pset, draws_dev, ndraws, to_host=True):
    """count -> allocate exact -> emit. Returns MeshResult (numpy copies when to_host)."""
    import torch
    sizes = tessellate_count(ctx, pset, draws_dev, ndraws)
    bufs = MeshBuffers(draws_dev.device, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    tessellate_emit(ctx, pset, draws_dev, ndraws, bufs)
    torch.cuda.synchronize()
    r = MeshResult()
    r.sizes = sizes
    r.bufs = bufs
    if to_host:
        nv, ni, nm = sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"]
        r.pos = bufs.pos[:nv].cpu().numpy()
        r.color = bufs.color[:nv].cpu().numpy().view(np.uint32)
        r.idx = bufs.idx[:ni].cpu().numpy().view(np.uint16)
        r.meshes = bufs.meshes[:nm * 32].cpu().numpy().view(capi.mesh_dtype)
    return r


def stroke(ctx, poly_dev, subs_dev, subdraw_dev, nsubs, draws_dev, ndraws, to_host=True):
    """Stroker-level entry (vgx_stroke_count + vgx_stroke_emit): already flattened + transformed vertex lists in,
    meshes out. poly_dev float32 [n,2], subs_dev uint8 (16-byte vgx_subpath records), subdraw_dev int32 [nsubs]."""
    import torch
    L = lib()
    sizes = capi.Sizes()
    s = _stream_ptr()
    _check(L.vgx_stroke_count(ctx.handle, poly_dev.data_ptr(), subs_dev.data_ptr(), subdraw_dev.data_ptr(), nsubs, draws_dev.data_ptr(), ndraws, C.byref(sizes), s), "vgx_stroke_count")
    sz = sizes.as_dict()
    bufs = MeshBuffers(poly_dev.device, sz["num_vertices"], sz["num_indices"], sz["num_meshes"])
    out = bufs.out_struct()
    _check(L.vgx_stroke_emit(ctx.handle, poly_dev.data_ptr(), subs_dev.data_ptr(), subdraw_dev.data_ptr(), nsubs, draws_dev.data_ptr(), ndraws, C.byref(out), s), "vgx_stroke_emit")
    torch.cuda.synchronize()
    r = MeshResult()
    r.sizes = sz
    r.bufs = bufs
    if to_host:
        nv, ni, nm = sz["num_vertices"], sz["num_indices"], sz["num_meshes"]
        r.pos = bufs.pos[:nv].cpu().numpy()
        r.color = bufs.color[:nv].cpu().numpy().view(np.uint32)
        r.idx = bufs.idx[:ni].cpu().numpy().view(np.uint16)
        r.meshes = bufs.meshes[:nm * 32].cpu().numpy().view(capi.mesh_dtype)
    return r


# ---- dashed strokes (vgx_dash): between flatten and the stroker-level entry ---------------------------------------------
class DashBuffers:
    """Caller-owned output buffers of vgx_dash in HBM (vgx_dash_out) + the device-side totals / status words."""

    def __init__(self, device, npoly, nsubs):
        import torch
        self.cap = (int(npoly), int(nsubs))
        self.poly = torch.empty((max(int(npoly), 1), 2), dtype=torch.float32, device=device)
        self.subs = torch.empty(max(int(nsubs), 1) * 16, dtype=torch.uint8, device=device)
        self.sub_draw = torch.empty(max(int(nsubs), 1), dtype=torch.int32, device=device)
        self.sub_src = torch.empty(max(int(nsubs), 1), dtype=torch.int32, device=device)
        self.dev_sizes = torch.zeros(10, dtype=torch.int64, device=device)
        self.dev_status = torch.zeros(1, dtype=torch.int32, device=device)

    def out_struct(self):
        return capi.DashOut(self.poly.data_ptr(), self.subs.data_ptr(), self.sub_draw.data_ptr(), self.sub_src.data_ptr(), self.cap[0], self.cap[1])


class DashResult:
    pass


def dash_validate(dashes, pattern):
    """vgx_dash_validate on host arrays (capi.dash_dtype records, float32 pattern). Returns the status."""
    d = np.ascontiguousarray(dashes)
    p = np.ascontiguousarray(pattern, dtype=np.float32)
    return int(lib().vgx_dash_validate(d.ctypes.data if d.size else None, d.shape[0], p.ctypes.data if p.size else None, p.shape[0]))


def subpath_draws(ctx, dinfo_dev, ndraws, nsubs):
    """vgx_subpath_draws: the draw of every sub-path of a flatten result (dinfo_dev: its 40-byte vgx_draw_info records). int32 [nsubs]."""
    import torch
    out = torch.empty(max(int(nsubs), 1), dtype=torch.int32, device=dinfo_dev.device)
    _check(lib().vgx_subpath_draws(ctx.handle, dinfo_dev.data_ptr(), ndraws, out.data_ptr(), nsubs, _stream_ptr()), "vgx_subpath_draws")
    return out


def dash_count(ctx, poly_dev, subs_dev, subdraw_dev, nsubs, dashes_dev, ndraws, pattern_dev, npattern):
    sizes = capi.Sizes()
    _check(lib().vgx_dash_count(ctx.handle, poly_dev.data_ptr(), subs_dev.data_ptr(), subdraw_dev.data_ptr(), nsubs, dashes_dev.data_ptr(), ndraws,
                                pattern_dev.data_ptr() if npattern else None, npattern, C.byref(sizes), _stream_ptr()), "vgx_dash_count")
    return sizes.as_dict()


def dash_async(ctx, poly_dev, subs_dev, subdraw_dev, nsubs, dashes_dev, ndraws, pattern_dev, npattern, bufs):
    """vgx_dash: single asynchronous call; totals / status land in bufs.dev_*."""
    out = bufs.out_struct()
    _check(lib().vgx_dash(ctx.handle, poly_dev.data_ptr(), subs_dev.data_ptr(), subdraw_dev.data_ptr(), nsubs, dashes_dev.data_ptr(), ndraws,
                          pattern_dev.data_ptr() if npattern else None, npattern, C.byref(out), bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(),
                          _stream_ptr()), "vgx_dash")


def dash(ctx, poly_dev, subs_dev, subdraw_dev, nsubs, dashes_dev, ndraws, pattern_dev, npattern, to_host=True):
    """count -> allocate exact -> vgx_dash. poly_dev float32 [n,2], subs_dev uint8 (16-byte vgx_subpath records), subdraw_dev int32
    [nsubs], dashes_dev uint8 (16-byte struct vgx_dash records, one per draw), pattern_dev float32 [npattern]. The pieces stay on
    the device (.poly_dev / .subs_dev / .sub_draw_dev / .sub_src_dev: what `stroke` takes) and come back as numpy copies when to_host."""
    import torch
    sizes = dash_count(ctx, poly_dev, subs_dev, subdraw_dev, nsubs, dashes_dev, ndraws, pattern_dev, npattern)
    npv, nsp = sizes["num_poly_vertices"], sizes["num_subpaths"]
    bufs = DashBuffers(poly_dev.device, npv, nsp)
    dash_async(ctx, poly_dev, subs_dev, subdraw_dev, nsubs, dashes_dev, ndraws, pattern_dev, npattern, bufs)
    torch.cuda.synchronize()
    st = int(bufs.dev_status.item())
    if st != capi.VGX_OK:
        raise VgxError(st, "vgx_dash (device)")
    r = DashResult()
    r.sizes = sizes
    r.bufs = bufs
    r.poly_dev, r.subs_dev, r.sub_draw_dev, r.sub_src_dev = bufs.poly, bufs.subs, bufs.sub_draw, bufs.sub_src
    if to_host:
        r.poly = bufs.poly[:npv].cpu().numpy()
        r.subpaths = bufs.subs[:nsp * 16].cpu().numpy().view(capi.subpath_dtype)
        r.sub_draw = bufs.sub_draw[:nsp].cpu().numpy().view(np.uint32)
        r.sub_src = bufs.sub_src[:nsp].cpu().numpy().view(np.uint32)
    return r


def stroke_async(ctx, poly_dev, subs_dev, subdraw_dev, nsubs, draws_dev, ndraws, bufs):
    """vgx_stroke: the stroker-level entry as one asynchronous call (the bytes of stroke()); totals / status land in bufs.dev_*."""
    out = bufs.out_struct()
    _check(lib().vgx_stroke(ctx.handle, poly_dev.data_ptr(), subs_dev.data_ptr(), subdraw_dev.data_ptr(), nsubs, draws_dev.data_ptr(), ndraws,
                            C.byref(out), bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_stroke")


# ---- dashed strokes in frames (vgx_tessellate_dashed): draws + one dash record per draw in, the frame's meshes out ----------
def tessellate_dashed_async(ctx, pset, draws_dev, ndraws, dashes_dev, pattern_dev, npattern, bufs, dev_dash_sizes=None):
    """vgx_tessellate_dashed: asynchronous like tessellate_immediate. dashes_dev uint8 (16-byte struct vgx_dash records, one per
    draw) or None, pattern_dev float32 [npattern]. The verdict lands in bufs.dev_status (VGX_OK / VGX_E_NOSPACE: grow the buffers
    to bufs.dev_sizes / VGX_E_GROWN: call again), the totals in bufs.dev_sizes, the pieces' totals in dev_dash_sizes (int64 [10])."""
    out = bufs.out_struct()
    _check(lib().vgx_tessellate_dashed(ctx.handle, pset.handle, draws_dev.data_ptr(), ndraws, dashes_dev.data_ptr() if dashes_dev is not None else None,
                                       pattern_dev.data_ptr() if npattern else None, npattern, C.byref(out), bufs.dev_sizes.data_ptr(),
                                       dev_dash_sizes.data_ptr() if dev_dash_sizes is not None else None, bufs.dev_status.data_ptr(), _stream_ptr()),
           "vgx_tessellate_dashed")


def tessellate_dashed(ctx, pset, draws_dev, ndraws, dashes_dev, pattern_dev, npattern, bufs=None, growth=1.5, max_calls=4, to_host=True):
    """The immediate-mode loop over tessellate_dashed_async (as tessellate_grow): until VGX_OK, growing the buffers after
    VGX_E_NOSPACE. Returns a MeshResult with .statuses (one per call), .sizes, .dash_sizes, .bufs and numpy copies when to_host."""
    import torch
    if bufs is None:
        bufs = MeshBuffers(draws_dev.device, 1024, 1024, 64)
    dds = torch.zeros(10, dtype=torch.int64, device=draws_dev.device)
    statuses = []
    for _ in range(max_calls):
        tessellate_dashed_async(ctx, pset, draws_dev, ndraws, dashes_dev, pattern_dev, npattern, bufs, dds)
        st = int(bufs.dev_status.item())  # (synchronises)
        statuses.append(st)
        sizes = capi.Sizes.from_buffer_copy(bufs.dev_sizes.cpu().numpy().tobytes()).as_dict()
        if st == capi.VGX_OK:
            r = MeshResult()
            r.statuses, r.sizes, r.bufs = statuses, sizes, bufs
            r.dash_sizes = capi.Sizes.from_buffer_copy(dds.cpu().numpy().tobytes()).as_dict()
            if to_host:
                nv, ni, nm = sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"]
                r.pos = bufs.pos[:nv].cpu().numpy()
                r.color = bufs.color[:nv].cpu().numpy().view(np.uint32)
                r.idx = bufs.idx[:ni].cpu().numpy().view(np.uint16)
                r.meshes = bufs.meshes[:nm * 32].cpu().numpy().view(capi.mesh_dtype)
            return r
        if st == capi.VGX_E_NOSPACE:
            nv, ni, nm = bufs.cap
            bufs = MeshBuffers(draws_dev.device, _grown(nv, sizes["num_vertices"], growth), _grown(ni, sizes["num_indices"], growth),
                               _grown(nm, sizes["num_meshes"], growth))
        elif st != capi.VGX_E_GROWN:
            raise VgxError(st, "vgx_tessellate_dashed (device)")
    raise VgxError(statuses[-1], "tessellate_dashed: no VGX_OK within %d calls (%s)" % (max_calls, statuses))


# ---- shape cache (vgx_cache_localize / vgx_cache_submit) ---------------------------------------------
class MeshCache:
    """A tessellated drawing kept in HBM in local space (the reference's CommandListCache, vg.cpp:249-256)."""

    def __init__(self, ctx, bufs, sizes, draws_dev, ndraws):
        """bufs: MeshBuffers that vgx_tessellate[_emit] filled for `draws_dev`; positions are localised in place."""
        self.bufs = bufs
        self.nv, self.ni, self.nm = int(sizes["num_vertices"]), int(sizes["num_indices"]), int(sizes["num_meshes"])
        _check(lib().vgx_cache_localize(ctx.handle, draws_dev.data_ptr(), ndraws, bufs.pos.data_ptr(), bufs.meshes.data_ptr(), self.nm, _stream_ptr()), "vgx_cache_localize")
        self._ctx = ctx
        self._bounds = None

    def desc(self):
        b = self.bufs
        return capi.CacheDesc(b.pos.data_ptr(), b.color.data_ptr(), b.idx.data_ptr(), b.meshes.data_ptr(), self.nm, self.nv, self.ni)

    @property
    def bounds(self):
        """float32 [nm, 4] device tensor: every mesh's local-space box (vgx_mesh_bounds), computed at the first use."""
        if self._bounds is None:
            self._bounds = mesh_bounds(self._ctx, self.bufs.pos, self.bufs.meshes, self.nm)
        return self._bounds


def cache_submit(ctx, cache, instances_dev, ninst, bufs):
    """instances_dev: uint8 device tensor of 40-byte vgx_cache_instance records. Asynchronous."""
    d = cache.desc()
    out = bufs.out_struct()
    _check(lib().vgx_cache_submit(ctx.handle, C.byref(d), instances_dev.data_ptr(), ninst, C.byref(out),
                                  bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_cache_submit")


# ---- bounding boxes and view culling (vgx_mesh_bounds / vgx_cache_cull) ------------------------------------------------
def mesh_bounds(ctx, pos, meshes, nm):
    """pos: float32 device tensor [nv, 2]; meshes: uint8 device tensor of 32-byte vgx_mesh records. Returns a float32 [nm, 4] device
    tensor (minx, miny, maxx, maxy per mesh). Asynchronous."""
    import torch
    out = torch.empty((max(int(nm), 1), 4), dtype=torch.float32, device=pos.device)[:nm]
    _check(lib().vgx_mesh_bounds(ctx.handle, pos.data_ptr(), meshes.data_ptr(), nm, out.data_ptr(), _stream_ptr()), "vgx_mesh_bounds")
    return out


class CullResult:
    """What vgx_cache_cull wrote, all on the device: inst (uint8 tensor of 40-byte records, same length and order as the input; the
    input tensor itself when in_place), bounds (float32 [ninst, 4] or None), kept (int32 [ninst] holding uint32 indices, the first
    num_kept are valid, or None), num_kept (int64 [1] or None), dev_status (int32 [1])."""


def cache_cull(ctx, cache, bounds_dev, inst_dev, ninst, views_dev, inst_view_dev=None, in_place=False, want_bounds=True, want_kept=True, reuse=None):
    """bounds_dev: the cache's per-mesh boxes (MeshCache.bounds); inst_dev: uint8 device tensor of 40-byte vgx_cache_instance records;
    views_dev: float32 [nviews, 4] (x0, y0, x1, y1); inst_view_dev: int32 / uint32 [ninst] or None (view 0). Asynchronous: hand
    result.inst to cache_submit with the same ninst. reuse: the CullResult of an earlier call for as many instances, written again
    instead of allocating (a frame loop); it decides which outputs exist, so in_place / want_bounds / want_kept must be left alone."""
    import torch
    dev = views_dev.device
    r = reuse
    if r is not None and (in_place or not want_bounds or not want_kept):
        raise ValueError("cache_cull: reuse= takes its outputs from the earlier result; do not combine it with in_place / want_*")
    if r is None:
        r = CullResult()
        r.inst = inst_dev if in_place else torch.empty(max(int(ninst), 1) * 40, dtype=torch.uint8, device=dev)
        r.bounds = torch.empty((max(int(ninst), 1), 4), dtype=torch.float32, device=dev) if want_bounds else None
        r.kept = torch.empty(max(int(ninst), 1), dtype=torch.int32, device=dev) if want_kept else None
        r.num_kept = torch.empty(1, dtype=torch.int64, device=dev) if want_kept else None
        r.dev_status = torch.empty(1, dtype=torch.int32, device=dev)
    d = cache.desc()

    def ptr(t):
        return t.data_ptr() if t is not None else None
    out = capi.CullOut(r.inst.data_ptr(), ptr(r.bounds), ptr(r.kept), ptr(r.num_kept))
    _check(lib().vgx_cache_cull(ctx.handle, C.byref(d), bounds_dev.data_ptr() if cache.nm else None, inst_dev.data_ptr() if ninst else None, ninst,
                                views_dev.data_ptr(), int(views_dev.shape[0]), ptr(inst_view_dev), C.byref(out), r.dev_status.data_ptr(), _stream_ptr()),
           "vgx_cache_cull")
    return r


# ---- what the frame consumers (vgx_pick*, vgx_raster*, vgx_damage_*) build alike -----------------------------------------
def _desc(frame):
    """A capi.CacheDesc of device pointers, or anything with .desc() (a MeshCache)."""
    return frame if isinstance(frame, capi.CacheDesc) else frame.desc()


def _ptr(t, used=True):
    """The device pointer of a tensor; None for None and for a table of no entries."""
    return t.data_ptr() if used and t is not None else None


def _mesh_end(mesh_end):
    """The end of a mesh range; None = open, every mesh from mesh_begin on."""
    return 0xFFFFFFFFFFFFFFFF if mesh_end is None else int(mesh_end)


def _hits(hits_dev, nqueries, device):
    import torch
    return torch.empty(max(int(nqueries), 1) * 16, dtype=torch.uint8, device=device) if hits_dev is None else hits_dev


def _raster_draws(draws_dev, draw_state_dev, num_draws):
    return capi.RasterDraws(_ptr(draws_dev, num_draws), _ptr(draw_state_dev, num_draws), int(num_draws), 0)


def _raster_target(pixels, width, height, stride, x0, y0, scissor=None, clear_color=None):
    sc = (0, 0, int(width), int(height)) if scissor is None else tuple(int(v) for v in scissor)
    return capi.RasterTarget(pixels, int(width), int(height), int(stride), int(x0), int(y0), (C.c_uint32 * 4)(*sc),
                             capi.RASTER_CLEAR if clear_color is not None else 0, int(clear_color or 0))


# ---- hit testing (vgx_pick) ---------------------------------------------------------------------------------------------
def pick(ctx, frame, queries_dev, nqueries, bounds_dev=None, hits_dev=None):
    """frame: a capi.CacheDesc of device pointers, or anything with .desc() (a MeshCache); queries_dev: uint8 device tensor of 16-byte
    vgx_pick_query records; bounds_dev: what mesh_bounds gave for the frame, or None (the call computes the boxes itself). Returns a
    uint8 device tensor of nqueries 16-byte vgx_pick_hit records (hits_dev when given). Asynchronous."""
    d = _desc(frame)
    hits_dev = _hits(hits_dev, nqueries, queries_dev.device)
    _check(lib().vgx_pick(ctx.handle, C.byref(d), _ptr(bounds_dev), queries_dev.data_ptr(), nqueries, hits_dev.data_ptr(), _stream_ptr()), "vgx_pick")
    return hits_dev


class PickRectResult:
    """What pick_rect() wrote, all device tensors: top (uint8, nqueries 16-byte vgx_pick_hit records, or None), list (int32
    [nqueries, list_cap], or None with list_cap == 0) and count (int32 [nqueries])."""

    def __init__(self, top, list_, count):
        self.top, self.list, self.count = top, list_, count


def pick_rect(ctx, frame, queries_dev, nqueries, list_cap=64, bounds_dev=None, want_top=True):
    """Rectangles against a frame: pick tolerance and marquee selection (vgx_pick_rect in include/vgx.h). frame: a capi.CacheDesc of device
    pointers, or anything with .desc(); queries_dev: uint8 device tensor of at most capi.PICK_RECT_MAX_QUERIES 32-byte vgx_pick_rect_query
    records; bounds_dev: what mesh_bounds gave for the frame, or None (the call computes the boxes itself). Returns a PickRectResult of
    device tensors: per query the number of selected entries, its list_cap lowest entries (only the first min(count, list_cap) of a row
    are written) and, with want_top, the topmost touching triangle of a selected entry. Asynchronous."""
    import torch
    d = _desc(frame)
    dev = queries_dev.device
    n, cap = max(int(nqueries), 1), int(list_cap)
    top = torch.empty(n * 16, dtype=torch.uint8, device=dev) if want_top else None
    lst = torch.empty((n, cap), dtype=torch.int32, device=dev) if cap else None
    count = torch.empty(n, dtype=torch.int32, device=dev)
    out = capi.PickRectOut(_ptr(top), _ptr(lst), count.data_ptr(), cap, 0)
    _check(lib().vgx_pick_rect(ctx.handle, C.byref(d), _ptr(bounds_dev), _ptr(queries_dev, nqueries), int(nqueries), C.byref(out), _stream_ptr()), "vgx_pick_rect")
    return PickRectResult(top, lst, count)


def pick_frame(ctx, frame, draws_dev, draw_state_dev, num_draws, queries_dev, nqueries, bounds_dev=None, mesh_begin=0, mesh_end=None, hits_dev=None,
               dev_status=None):
    """pick() for the image raster_concave() draws: a mesh is hit where a sample of it would take effect under its draw's scissor and the
    clip region its draw names, the meshes of Clip draws stamp and are never hit, a mesh of kind capi.MESH_CONTOURS is hit by its winding
    rule (triangle = capi.PICK_NONE), and a point on a seam names the triangle the image draws (vgx_pick_frame in include/vgx.h).
    draws_dev / draw_state_dev / num_draws as in raster_frame(); the mesh range must hold the clip meshes of every region it uses.
    Returns (hits, dev_status): a uint8 device tensor of nqueries 16-byte vgx_pick_hit records (hits_dev when given) and an int32 [1]
    tensor that holds VGX_OK, or VGX_E_INVALID_ARG when a mesh names a draw >= num_draws (every hit is "none" then). Asynchronous."""
    import torch
    d = _desc(frame)
    hits_dev = _hits(hits_dev, nqueries, queries_dev.device)
    if dev_status is None:
        dev_status = torch.empty(1, dtype=torch.int32, device=hits_dev.device)
    st = _raster_draws(draws_dev, draw_state_dev, num_draws)
    _check(lib().vgx_pick_frame(ctx.handle, C.byref(d), _ptr(bounds_dev), int(mesh_begin), _mesh_end(mesh_end), C.byref(st), _ptr(queries_dev, nqueries),
                                int(nqueries), hits_dev.data_ptr(), dev_status.data_ptr(), _stream_ptr()), "vgx_pick_frame")
    return hits_dev, dev_status


# ---- rendering to an image (vgx_raster) -----------------------------------------------------------------------------------
def _raster(entry, ctx, frame, width, height, x0, y0, scissor, clear_color, bounds_dev, mesh_begin, mesh_end, image, dev_status, draws=None, textures=None,
            paints=None, damage=None):
    """The body of every raster call: `entry` of libvgx.so on the target and, in the order of the entry's parameters, the structs of the
    tables it takes -- draws (draws_dev, draw_state_dev, num_draws), textures (uv_dev, uv_bytes, images_dev, num_images), paints
    (gradients_dev, num_gradients, patterns_dev, num_patterns), damage (tile_bits, max_entries); None = not a parameter of that entry.
    Allocates the image and the status word nobody handed in. Returns (image, dev_status)."""
    import torch
    d = _desc(frame)
    if image is None:
        image = torch.zeros((max(int(height), 1), max(int(width), 1)), dtype=torch.int32, device="cuda:%d" % ctx.device)[:height, :width]
    if dev_status is None:
        dev_status = torch.empty(1, dtype=torch.int32, device=image.device)
    structs = []
    if draws is not None:
        structs.append(_raster_draws(*draws))
    if textures is not None:
        uv_dev, uv_bytes, images_dev, num_images = textures
        structs.append(capi.RasterTextures(_ptr(uv_dev), _ptr(images_dev, num_images), int(uv_bytes), int(num_images)))
    if paints is not None:
        gradients_dev, num_gradients, patterns_dev, num_patterns = paints
        structs.append(capi.RasterPaints(_ptr(gradients_dev, num_gradients), _ptr(patterns_dev, num_patterns), int(num_gradients), int(num_patterns)))
    structs.append(_raster_target(image.data_ptr(), width, height, image.stride(0) if image.dim() == 2 and height else width, x0, y0, scissor, clear_color))
    if damage is not None:
        structs.append(capi.RasterDamage(damage[0].data_ptr(), int(damage[1]), 0))
    _check(getattr(lib(), entry)(ctx.handle, C.byref(d), _ptr(bounds_dev), int(mesh_begin), _mesh_end(mesh_end), *[C.byref(s) for s in structs],
                                 dev_status.data_ptr(), _stream_ptr()), entry)
    return image, dev_status


def raster(ctx, frame, width, height, x0=0, y0=0, scissor=None, clear_color=None, bounds_dev=None, mesh_begin=0, mesh_end=None, image=None,
           dev_status=None):
    """Draws the meshes [mesh_begin, mesh_end) of `frame` (a capi.CacheDesc of device pointers, or anything with .desc()) into an RGBA8
    image on the device: pixel (i, j) samples the frame at (x0 + i + 0.5, y0 + j + 0.5). scissor: (sx0, sy0, sx1, sy1) in image pixels,
    None = the whole image; clear_color: 0xAABBGGRR the scissor is set to first, None = drawn over what `image` holds (zeros for a new
    one); bounds_dev: what mesh_bounds gave for the frame, or None. image: an int32 [height, stride] device tensor to draw into
    (stride = its row length). Returns (image, dev_status): the int32 tensor whose words are 0xAABBGGRR and an int32 [1] tensor that
    holds VGX_OK, VGX_E_GROWN (call again) or VGX_E_RANGE once the work is done. Asynchronous."""
    return _raster("vgx_raster", ctx, frame, width, height, x0, y0, scissor, clear_color, bounds_dev, mesh_begin, mesh_end, image, dev_status)


def raster_frame(ctx, frame, draws_dev, draw_state_dev, num_draws, width, height, x0=0, y0=0, scissor=None, clear_color=None, bounds_dev=None,
                 mesh_begin=0, mesh_end=None, image=None, dev_status=None):
    """raster() under the state of a decoded frame: draws_dev / draw_state_dev are uint8 device tensors of num_draws 64-byte vgx_draw and
    24-byte vgx_draw_state records (what cmdlist decoding gave), indexed by the meshes' draw. Every mesh is cut by its draw's scissor,
    clip draws stamp their region, the other draws are tested against the region they name (vgx_raster_frame in include/vgx.h). The
    mesh range must hold the clip meshes of every region it uses. dev_status may also come out as VGX_E_INVALID_ARG: a mesh names a
    draw >= num_draws, nothing was written. Returns (image, dev_status) as raster() does. Asynchronous."""
    return _raster("vgx_raster_frame", ctx, frame, width, height, x0, y0, scissor, clear_color, bounds_dev, mesh_begin, mesh_end, image, dev_status,
                   draws=(draws_dev, draw_state_dev, num_draws))


def raster_images(images, device):
    """The image table of raster_textured() in device memory: `images` is a list of (pixels, flags) with pixels an int32 [height, stride]
    device tensor of 0xAABBGGRR texels (width = its column count; a view of a wider tensor gives stride > width) and flags the
    capi.IMAGE_* bits. Returns a uint8 device tensor of 24-byte vgx_raster_image records; the caller keeps the pixel tensors alive."""
    import numpy as np
    import torch
    rec = np.zeros(len(images), dtype=capi.raster_image_dtype)
    for k, (px, flags) in enumerate(images):
        rec[k] = (px.data_ptr(), int(px.shape[1]), int(px.shape[0]), int(px.stride(0)), int(flags))
    return torch.from_numpy(rec.view(np.uint8).copy()).to(device)


def raster_textured(ctx, frame, draws_dev, draw_state_dev, num_draws, uv_dev, uv_bytes, images_dev, num_images, width, height, x0=0, y0=0, scissor=None,
                    clear_color=None, bounds_dev=None, mesh_begin=0, mesh_end=None, image=None, dev_status=None):
    """raster_frame() that also draws text and user meshes: a mesh of kind TEXT or TRILIST under a draw of type 0 is sampled from the
    image its draw names (state_key & 0xFFFF indexes images_dev, what raster_images() gave) with the UVs of uv_dev, a device tensor
    of uv_bytes (4: int16 x 2, 8: float x 2) per vertex of the frame, read only at the vertices of sampled meshes
    (vgx_raster_textured in include/vgx.h). dev_status may also come out as VGX_E_INVALID_ARG for a sampled mesh whose handle or
    image record is no good: nothing was written. Returns (image, dev_status) as raster() does. Asynchronous."""
    return _raster("vgx_raster_textured", ctx, frame, width, height, x0, y0, scissor, clear_color, bounds_dev, mesh_begin, mesh_end, image, dev_status,
                   draws=(draws_dev, draw_state_dev, num_draws), textures=(uv_dev, uv_bytes, images_dev, num_images))


def paint_tables(paints, num_gradients=None, num_patterns=None):
    """vgx_paint_tables: scatters the vgx_paint records vgx_cmdlist_decode wrote (a capi.paint_dtype array) into the gradient table and
    the pattern table raster_painted() indexes by handle; entries no record names have type capi.PAINT_UNUSED. The sizes default to
    the highest handle of each type plus one. Returns (gradients, patterns) as capi.paint_dtype arrays. Host only."""
    import numpy as np
    paints = np.ascontiguousarray(paints, dtype=capi.paint_dtype)
    caps = []
    for given, t in ((num_gradients, capi.DRAW_TYPE_GRADIENT), (num_patterns, capi.DRAW_TYPE_PATTERN)):
        h = paints["handle"][paints["type"] == t]
        caps.append(int(given) if given is not None else (int(h.max()) + 1 if h.size else 0))
    g, p = np.zeros(max(caps[0], 1), capi.paint_dtype), np.zeros(max(caps[1], 1), capi.paint_dtype)
    _check(lib().vgx_paint_tables(paints.ctypes.data if paints.shape[0] else None, int(paints.shape[0]), g.ctypes.data, caps[0], p.ctypes.data, caps[1]),
           "vgx_paint_tables")
    return g[:caps[0]], p[:caps[1]]


def raster_painted(ctx, frame, draws_dev, draw_state_dev, num_draws, uv_dev, uv_bytes, images_dev, num_images, gradients_dev, num_gradients, patterns_dev,
                   num_patterns, width, height, x0=0, y0=0, scissor=None, clear_color=None, bounds_dev=None, mesh_begin=0, mesh_end=None, image=None,
                   dev_status=None, _entry="vgx_raster_painted"):
    """raster_textured() that also paints: a mesh whose draw has type 1 (ColorGradient) or 2 (ImagePattern) takes its colour from the
    vgx_paint record its draw names (state_key & 0xFFFF indexes gradients_dev / patterns_dev, the tables of paint_tables() as uint8
    device tensors; a pattern's .image indexes images_dev) by the fragment rule of vgx_raster_painted in include/vgx.h. dev_status may
    also come out as VGX_E_INVALID_ARG for a painted mesh whose handle, table entry or image is no good: nothing was written.
    Returns (image, dev_status) as raster() does. Asynchronous."""
    return _raster(_entry, ctx, frame, width, height, x0, y0, scissor, clear_color, bounds_dev, mesh_begin, mesh_end, image, dev_status,
                   draws=(draws_dev, draw_state_dev, num_draws), textures=(uv_dev, uv_bytes, images_dev, num_images),
                   paints=(gradients_dev, num_gradients, patterns_dev, num_patterns))


def raster_concave(*args, **kwargs):
    """raster_painted() that also fills meshes of kind capi.MESH_CONTOURS (what concave_contours() writes) by the winding number of
    their edges: the rule of vgx_raster_concave in include/vgx.h. Same arguments and results as raster_painted()."""
    return raster_painted(*args, _entry="vgx_raster_concave", **kwargs)


def raster_reserve(ctx, num_meshes, num_bin_entries):
    """Sizes the scratch of raster(), raster_frame(), raster_textured(), raster_painted() and raster_concave() ahead, so that a first call does not end with VGX_E_GROWN."""
    _check(lib().vgx_raster_reserve(ctx.handle, int(num_meshes), int(num_bin_entries)), "vgx_raster_reserve")


# ---- a draw-command table to an image (vgx_raster_commands) ----------------------------------------------------------------
def raster_streams(pos_dev, color_dev, idx_dev, num_vertices, num_indices, uv_dev=None, uv_bytes=0):
    """The capi.RasterStreams of an assembled frame: pos / color / idx (and uv, uv_bytes 4 or 8 per vertex) device tensors, as
    MeshBuffers holds them after a tessellate call under set_assembly; idx is command-relative."""
    return capi.RasterStreams(_ptr(pos_dev, num_vertices), _ptr(color_dev, num_vertices), _ptr(uv_dev), _ptr(idx_dev, num_indices), int(num_vertices), int(num_indices),
                              int(uv_bytes) if uv_dev is not None else 0, 0)


def raster_commands(ctx, streams, cmds_dev, num_cmds, width, height, images_dev=None, num_images=0, gradients_dev=None, num_gradients=0, patterns_dev=None,
                    num_patterns=0, x0=0, y0=0, scissor=None, clear_color=None, dev_num_cmds=None, image=None, dev_status=None, _damage=None):
    """Draws a draw-command table into an RGBA8 image on the device: cmds_dev is a uint8 device tensor of num_cmds 56-byte vgx_raster_cmd
    records (capi.raster_cmd_dtype; what raster_cmds_from_assembly() wrote, or the reference's tables through submit_order()), streams a
    capi.RasterStreams (raster_streams()). Command c is cut by its scissor, stamps its index (type 3) or is tested against the command
    range it names, and is sampled (type 0, images_dev as raster_images() gave), painted (types 1 / 2, the tables of paint_tables(); with
    both counts 0 no paints are handed in) by the rule of vgx_raster_commands in include/vgx.h. dev_num_cmds: an int32 [1] device
    tensor with the real count, or None. Returns (image, dev_status) as raster() does; dev_status may hold VGX_OK, VGX_E_GROWN (call
    again), VGX_E_INVALID_ARG or VGX_E_RANGE. Asynchronous."""
    import torch
    if image is None:
        image = torch.zeros((max(int(height), 1), max(int(width), 1)), dtype=torch.int32, device="cuda:%d" % ctx.device)[:height, :width]
    if dev_status is None:
        dev_status = torch.empty(1, dtype=torch.int32, device=image.device)
    paints = capi.RasterPaints(_ptr(gradients_dev, num_gradients), _ptr(patterns_dev, num_patterns), int(num_gradients), int(num_patterns))
    tgt = _raster_target(image.data_ptr(), width, height, image.stride(0) if image.dim() == 2 and height else width, x0, y0, scissor, clear_color)
    # _damage = (tile_bits, max_entries, bounds_dev): the arguments the damaged entry adds -- the boxes behind dev_num_cmds, the struct behind the target
    entry = "vgx_raster_commands" if _damage is None else "vgx_raster_commands_damaged"
    boxes = () if _damage is None else (_ptr(_damage[2], num_cmds),)
    dmg = () if _damage is None else (C.byref(capi.RasterDamage(_damage[0].data_ptr(), int(_damage[1]), 0)),)
    _check(getattr(lib(), entry)(ctx.handle, C.byref(streams), _ptr(cmds_dev, num_cmds), int(num_cmds), _ptr(dev_num_cmds), *boxes, _ptr(images_dev, num_images),
                                 int(num_images), C.byref(paints) if (num_gradients or num_patterns) else None, C.byref(tgt), *dmg, dev_status.data_ptr(), _stream_ptr()),
           entry)
    return image, dev_status


def raster_commands_damaged(ctx, streams, cmds_dev, num_cmds, width, height, tile_bits, image, bounds_dev=None, max_entries=0, **kwargs):
    """raster_commands() into `image` (the int32 [height, stride] device tensor an earlier render left), restricted to the tiles whose bit
    is set in tile_bits (damage_meshes() / damage_instances() marks; damage_meshes() takes the table of command_bounds() as its box
    table). bounds_dev: what command_bounds() gives for the table, or None; with it a command whose box reaches no marked tile is not
    opened. With clear_color given, and every tile marked that the old or the new box of an edited command reaches, the image equals a
    full raster_commands() of the edited table (vgx_raster_commands_damaged in include/vgx.h). max_entries: the bin entries the call
    sorts at most, 0 = what the last damaged commands call on this context needed. dev_status may come out as VGX_E_GROWN: call again.
    Other arguments and the results as raster_commands(). Asynchronous."""
    return raster_commands(ctx, streams, cmds_dev, num_cmds, width, height, image=image, _damage=(tile_bits, max_entries, bounds_dev), **kwargs)


def raster_commands_reserve(ctx, num_cmds, num_chunks, num_bin_entries):
    """Sizes the scratch of raster_commands() ahead (chunks of capi.RASTER_CHUNK triangles, pairs of a chunk and a tile), so that a first
    call does not end with VGX_E_GROWN."""
    _check(lib().vgx_raster_commands_reserve(ctx.handle, int(num_cmds), int(num_chunks), int(num_bin_entries)), "vgx_raster_commands_reserve")


def raster_cmds_from_assembly(ctx, drawcmds_dev, cap_drawcmds, dev_num_drawcmds, meshes_dev, num_meshes, draw_state_dev, num_draws, out_dev=None):
    """The product's own assembled frame as a command table, on the device: drawcmds_dev / dev_num_drawcmds are what an assembly armed
    with capi.ASM_SPLIT_STATE wrote (48-byte vgx_drawcmd records, an int64 [1] count or None), meshes_dev the frame's mesh table,
    draw_state_dev the decoder's 24-byte vgx_draw_state records. Returns (cmds, dev_num_cmds, dev_status): a uint8 device tensor of
    cap_drawcmds 56-byte vgx_raster_cmd records (out_dev when given), an int32 [1] count and an int32 [1] status (VGX_OK, or
    VGX_E_INVALID_ARG for a command outside its tables or a frame with contour meshes). Asynchronous."""
    import torch
    dev = drawcmds_dev.device
    if out_dev is None:
        out_dev = torch.empty(max(int(cap_drawcmds), 1) * capi.raster_cmd_dtype.itemsize, dtype=torch.uint8, device=dev)
    n, status = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    st = _raster_draws(None, draw_state_dev, num_draws)
    _check(lib().vgx_raster_cmds_from_assembly(ctx.handle, _ptr(drawcmds_dev, cap_drawcmds), int(cap_drawcmds), _ptr(dev_num_drawcmds), _ptr(meshes_dev, num_meshes),
                                               int(num_meshes), C.byref(st), out_dev.data_ptr(), n.data_ptr(), status.data_ptr(), _stream_ptr()),
           "vgx_raster_cmds_from_assembly")
    return out_dev, n, status


def submit_order(draw_cmds, clip_cmds):
    """vgx_submit_order: the reference's two command tables (capi.raster_cmd_dtype arrays; a draw command's clip range indexes clip_cmds)
    as ONE table in the order vg::end submits them: the clip commands of a region, as type 3, ahead of the first command that uses it,
    again after every interruption, and the users' ranges rewritten to where the copies landed. Host only."""
    import numpy as np
    d = np.ascontiguousarray(draw_cmds, dtype=capi.raster_cmd_dtype)
    c = np.ascontiguousarray(clip_cmds, dtype=capi.raster_cmd_dtype)
    n = C.c_uint32(0)
    args = (d.ctypes.data if d.shape[0] else None, int(d.shape[0]), c.ctypes.data if c.shape[0] else None, int(c.shape[0]))
    st = lib().vgx_submit_order(*args, None, 0, C.byref(n))
    if st not in (capi.VGX_OK, capi.VGX_E_NOSPACE):
        _check(st, "vgx_submit_order")
    out = np.zeros(max(n.value, 1), dtype=capi.raster_cmd_dtype)
    _check(lib().vgx_submit_order(*args, out.ctypes.data, n.value, C.byref(n)), "vgx_submit_order")
    return out[:n.value]


# ---- hit testing of a draw-command table (vgx_pick_commands) -----------------------------------------------------------------
def pick_commands(ctx, streams, cmds_dev, num_cmds, queries_dev, nqueries, meshes_dev=None, num_meshes=0, dev_num_cmds=None, hits_dev=None, dev_status=None,
                  _boxed=False, _bounds=None):
    """pick_frame() for the image raster_commands() draws: streams (raster_streams()) and cmds_dev as there; queries_dev a uint8 device
    tensor of nqueries 24-byte vgx_pick_cmd_query records (capi.pick_cmd_query_dtype: the point, the (cmd_end, tri_end) limit below which
    hits count -- cmd_end = capi.PICK_NONE: everything -- and the flags of pick()). meshes_dev / num_meshes: the mesh table of the
    assembled frame, which names the mesh and the draw that own the hit triangle, or None. Returns (hits, dev_status): a uint8 device
    tensor of nqueries 16-byte vgx_pick_cmd_hit records (capi.pick_cmd_hit_dtype; hits_dev when given) and an int32 [1] tensor that holds
    VGX_OK, or VGX_E_INVALID_ARG for an invalid record of the table (every hit is "none" then). Asynchronous."""
    import torch
    dev = queries_dev.device if queries_dev is not None else "cuda:%d" % ctx.device
    hits_dev = _hits(hits_dev, nqueries, dev)
    if dev_status is None:
        dev_status = torch.empty(1, dtype=torch.int32, device=hits_dev.device)
    owners = capi.PickOwners(_ptr(meshes_dev, num_meshes), int(num_meshes)) if meshes_dev is not None else None
    entry = "vgx_pick_commands_boxed" if _boxed else "vgx_pick_commands"
    boxes = (_ptr(_bounds, num_cmds),) if _boxed else ()   # the one argument the boxed entry adds, behind dev_num_cmds
    _check(getattr(lib(), entry)(ctx.handle, C.byref(streams), _ptr(cmds_dev, num_cmds), int(num_cmds), _ptr(dev_num_cmds), *boxes, C.byref(owners) if owners is not None else None,
                                 _ptr(queries_dev, nqueries), int(nqueries), hits_dev.data_ptr(), dev_status.data_ptr(), _stream_ptr()), entry)
    return hits_dev, dev_status


def pick_commands_boxed(ctx, streams, cmds_dev, num_cmds, bounds_dev, queries_dev, nqueries, **kwargs):
    """pick_commands() that never opens a command whose box misses the point: bounds_dev is the float32 [num_cmds, 4] table
    command_bounds() gave for the table, or None (then it is pick_commands()). True boxes change no answer; what the table holds decides
    (the rule of vgx_pick_commands_boxed in include/vgx.h). Other arguments and the results as pick_commands()."""
    return pick_commands(ctx, streams, cmds_dev, num_cmds, queries_dev, nqueries, _boxed=True, _bounds=bounds_dev, **kwargs)


# ---- boxes of a draw-command table (vgx_command_bounds) -------------------------------------------------------------------------
def command_bounds(ctx, streams, cmds_dev, num_cmds, cmd_begin=0, cmd_end=None, dev_num_cmds=None, bounds_dev=None, dev_status=None):
    """The box of every command of a draw-command table over the corners of its triangles: streams (raster_streams()) and cmds_dev as
    raster_commands() takes them. Writes the entries [cmd_begin, min(cmd_end, real count)) of bounds_dev, a float32 [num_cmds, 4] device
    tensor (allocated, every entry the empty box, when None), and leaves the others alone: after an edit of a few commands only those
    are refreshed. Returns (bounds, dev_status): minx, miny, maxx, maxy per command, (+inf, +inf, -inf, -inf) for one without a
    triangle, and an int32 [1] tensor that holds VGX_OK, or VGX_E_INVALID_ARG for a record of the range whose ranges leave the streams
    (it gets the empty box). No precondition on order or overlap of the commands' ranges. Asynchronous."""
    import torch
    dev = cmds_dev.device if cmds_dev is not None else "cuda:%d" % ctx.device
    if bounds_dev is None:
        inf = float("inf")
        bounds_dev = torch.tensor([inf, inf, -inf, -inf], dtype=torch.float32, device=dev).repeat(max(int(num_cmds), 1), 1)[:int(num_cmds)]
    if dev_status is None:
        dev_status = torch.empty(1, dtype=torch.int32, device=dev)
    end = 0xFFFFFFFF if cmd_end is None else int(cmd_end)
    _check(lib().vgx_command_bounds(ctx.handle, C.byref(streams), _ptr(cmds_dev, num_cmds), int(num_cmds), _ptr(dev_num_cmds), int(cmd_begin), end,
                                    _ptr(bounds_dev, num_cmds), dev_status.data_ptr(), _stream_ptr()), "vgx_command_bounds")
    return bounds_dev, dev_status


# ---- incremental update (vgx_cache_layout / vgx_cache_update) ------------------------------------------------------------
def cache_layout(ctx, cache, inst_dev, ninst, slots_dev=None):
    """Where every instance of `inst_dev` (uint8 device tensor of 40-byte vgx_cache_instance records) lives in the frame cache_submit
    writes for it. Returns (slots, dev_status): a uint8 device tensor of ninst + 1 32-byte vgx_cache_slot records (slots_dev when
    given) and an int32 [1] device tensor. Asynchronous."""
    import torch
    dev = cache.bufs.pos.device
    if slots_dev is None:
        slots_dev = torch.empty((int(ninst) + 1) * 32, dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    d = cache.desc()
    _check(lib().vgx_cache_layout(ctx.handle, C.byref(d), inst_dev.data_ptr() if ninst else None, ninst, slots_dev.data_ptr(), status.data_ptr(),
                                  _stream_ptr()), "vgx_cache_layout")
    return slots_dev, status


def cache_update(ctx, cache, inst_dev, ninst, slots_dev, dirty_dev, ndirty, pos, color, num_vertices, num_meshes, mesh_bounds=None,
                 dev_ndirty=None, dev_status=None):
    """Rewrites the slices of the listed instances in a frame cache_submit wrote. inst_dev: the EDITED instance array; slots_dev: what
    cache_layout gave for the submitted one; dirty_dev: int32 / uint32 device tensor of instance indices, the first ndirty (or
    min(ndirty, dev_ndirty[0]), dev_ndirty an int64 [1] device tensor) are used; pos / color: the frame's streams (MeshBuffers.pos /
    .color); mesh_bounds: the float32 [num_meshes, 4] table mesh_bounds() gave for the frame, refreshed in place, or None. Returns
    dev_status (int32 [1] device tensor: VGX_OK, VGX_E_INVALID_ARG or VGX_E_STALE). Asynchronous."""
    import torch
    if dev_status is None:
        dev_status = torch.empty(1, dtype=torch.int32, device=pos.device)
    d = cache.desc()
    fr = capi.UpdateFrame(pos.data_ptr(), color.data_ptr(), int(num_vertices), int(num_meshes), mesh_bounds.data_ptr() if mesh_bounds is not None else None)
    _check(lib().vgx_cache_update(ctx.handle, C.byref(d), inst_dev.data_ptr() if ninst else None, ninst, slots_dev.data_ptr(),
                                  dirty_dev.data_ptr() if ndirty else None, ndirty, dev_ndirty.data_ptr() if dev_ndirty is not None else None,
                                  C.byref(fr), dev_status.data_ptr(), _stream_ptr()), "vgx_cache_update")
    return dev_status


# ---- damage redraw (vgx_damage_* / vgx_raster_damaged) ---------------------------------------------------------------------
def damage_words(width, height):
    """uint32 words of the damage bitmap of a width x height image: one bit per 16 x 16 tile. Host only."""
    return int(lib().vgx_damage_words(int(width), int(height)))


def _damage_target(width, height, x0, y0):
    return _raster_target(None, width, height, width, x0, y0)


def damage_meshes(ctx, bounds_dev, num_meshes, width, height, tile_bits, x0=0, y0=0, mesh_begin=0, mesh_end=None):
    """ORs into tile_bits (an int32 device tensor of damage_words(width, height) words the caller zeroed) the tiles the boxes of meshes
    [mesh_begin, mesh_end) of bounds_dev (float32 [num_meshes, 4], what mesh_bounds() gave) reach in the image raster_damaged() will
    draw: same width, height, x0, y0. Returns tile_bits. Asynchronous."""
    t = _damage_target(width, height, x0, y0)
    _check(lib().vgx_damage_meshes(ctx.handle, _ptr(bounds_dev, num_meshes), int(mesh_begin), _mesh_end(mesh_end), int(num_meshes), C.byref(t),
                                   tile_bits.data_ptr(), _stream_ptr()), "vgx_damage_meshes")
    return tile_bits


def damage_instances(ctx, bounds_dev, num_meshes, slots_dev, ninst, dirty_dev, ndirty, width, height, tile_bits, x0=0, y0=0, dev_ndirty=None,
                     dev_status=None):
    """ORs into tile_bits the tiles the boxes of the frame meshes of the listed instances reach: slots_dev / dirty_dev / ndirty /
    dev_ndirty as in cache_update(), bounds_dev the frame's box table. Call it before cache_update() (the old boxes) and after it (the
    new ones, the table cache_update() refreshed). Returns dev_status (int32 [1] device tensor: VGX_OK, or VGX_E_INVALID_ARG when an
    entry was skipped). Asynchronous."""
    import torch
    if dev_status is None:
        dev_status = torch.empty(1, dtype=torch.int32, device=tile_bits.device)
    t = _damage_target(width, height, x0, y0)
    _check(lib().vgx_damage_instances(ctx.handle, _ptr(bounds_dev, num_meshes), int(num_meshes), slots_dev.data_ptr(), int(ninst), _ptr(dirty_dev, ndirty),
                                      int(ndirty), _ptr(dev_ndirty), C.byref(t), tile_bits.data_ptr(), dev_status.data_ptr(), _stream_ptr()), "vgx_damage_instances")
    return dev_status


def raster_damaged(ctx, frame, draws_dev, draw_state_dev, num_draws, uv_dev, uv_bytes, images_dev, num_images, gradients_dev, num_gradients, patterns_dev,
                   num_patterns, width, height, tile_bits, image, max_entries=0, x0=0, y0=0, scissor=None, clear_color=None, bounds_dev=None, mesh_begin=0,
                   mesh_end=None, dev_status=None):
    """raster_concave() into `image` (the int32 [height, stride] device tensor an earlier render left), restricted to the tiles whose bit
    is set in tile_bits: with clear_color given, and every tile marked that the old or the new box of an edited mesh reaches, the image
    equals a full raster_concave() of the edited frame (vgx_raster_damaged in include/vgx.h). max_entries: the bin entries the call sorts
    at most, 0 = what the last damaged call on this context needed. dev_status may come out as VGX_E_GROWN: call again. Returns
    (image, dev_status). Asynchronous."""
    return _raster("vgx_raster_damaged", ctx, frame, width, height, x0, y0, scissor, clear_color, bounds_dev, mesh_begin, mesh_end, image, dev_status,
                   draws=(draws_dev, draw_state_dev, num_draws), textures=(uv_dev, uv_bytes, images_dev, num_images),
                   paints=(gradients_dev, num_gradients, patterns_dev, num_patterns), damage=(tile_bits, max_entries))


# ---- concave fills (vgx_concave_move / vgx_concave_emit): libtess2 stays with the caller -----------------------------
def concave_move(ctx, contour_verts_dev, contours_dev, ncontours, fills_dev, nfills):
    """Inner fringe vertex of every boundary-contour vertex (what the reference writes back into the contour before the
    second libtess2 pass). contour_verts_dev float32 [n,2]; contours_dev / fills_dev uint8 tensors of 16-byte vgx_contour /
    48-byte vgx_concave_fill records. Returns a float32 [n,2] device tensor."""
    import torch
    n = int(contour_verts_dev.shape[0])
    moved = torch.empty_like(contour_verts_dev)
    _check(lib().vgx_concave_move(ctx.handle, contour_verts_dev.data_ptr(), n, contours_dev.data_ptr(), ncontours,
                                  fills_dev.data_ptr(), nfills, moved.data_ptr(), _stream_ptr()), "vgx_concave_move")
    return moved


def concave_emit(ctx, contour_verts_dev, contours_dev, ncontours, fills_dev, nfills, tess_pos_dev, tess_idx_dev, bufs):
    """One mesh per fill: fringe + interior (see include/vgx.h). Asynchronous; totals / status land in bufs.dev_*."""
    n = int(contour_verts_dev.shape[0])
    out = bufs.out_struct()
    _check(lib().vgx_concave_emit(ctx.handle, contour_verts_dev.data_ptr(), n, contours_dev.data_ptr(), ncontours,
                                  fills_dev.data_ptr(), nfills, tess_pos_dev.data_ptr(), tess_idx_dev.data_ptr(), C.byref(out),
                                  bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_concave_emit")


def concave_contours(ctx, poly_dev, subpaths_dev, draw_info_dev, draws_dev, ndraws, bufs):
    """Contour meshes for the concave draws of a frame, without libtess2 (vgx_concave_contours in include/vgx.h). poly_dev,
    subpaths_dev, draw_info_dev: what flatten wrote with apply_transform = 1, as device tensors; draws_dev: the frame's 64-byte vgx_draw
    records. The meshes (ascending by draw: sequence b of merge()) go to `bufs`. Asynchronous; totals / status land in bufs.dev_*."""
    out = bufs.out_struct()
    _check(lib().vgx_concave_contours(ctx.handle, poly_dev.data_ptr() if ndraws else None, subpaths_dev.data_ptr() if ndraws else None,
                                      draw_info_dev.data_ptr() if ndraws else None, draws_dev.data_ptr() if ndraws else None, int(ndraws), C.byref(out),
                                      bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_concave_contours")


def concave_triangulate(ctx, poly_dev, subpaths_dev, draw_info_dev, draws_dev, ndraws, bufs, draw_route=None):
    """concave_contours() whose draws of ONE simple ring come out as triangles -- ear clipping on the device, one mesh of kind
    capi.MESH_CONCAVE_FILL_AA each -- while every other concave draw keeps its contour meshes (vgx_concave_triangulate in include/vgx.h).
    Returns the int32 [ndraws] device tensor of routes (draw_route, or a new one): 0 = no mesh, capi.TRI_ROUTE_TRIANGLES, or a
    capi.TRI_REFUSED_* reason. Asynchronous; totals / status land in bufs.dev_*."""
    import torch
    if draw_route is None:
        draw_route = torch.zeros(max(int(ndraws), 1), dtype=torch.int32, device=bufs.dev_status.device)
    out = bufs.out_struct()
    _check(lib().vgx_concave_triangulate(ctx.handle, poly_dev.data_ptr() if ndraws else None, subpaths_dev.data_ptr() if ndraws else None,
                                         draw_info_dev.data_ptr() if ndraws else None, draws_dev.data_ptr() if ndraws else None, int(ndraws), C.byref(out),
                                         draw_route.data_ptr(), bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_concave_triangulate")
    return draw_route


def concave_triangulate_rings(ctx, poly_dev, subpaths_dev, draw_info_dev, draws_dev, ndraws, bufs, draw_route=None):
    """concave_triangulate() that also triangulates a draw of several sub-paths when they are one outer ring with holes directly inside
    it (vgx_concave_triangulate_rings in include/vgx.h). The routes never hold capi.TRI_REFUSED_MULTI; such a draw is triangulated or
    refused as capi.TRI_REFUSED_NESTING / TRI_REFUSED_NO_BRIDGE or one of the single-ring reasons."""
    import torch
    if draw_route is None:
        draw_route = torch.zeros(max(int(ndraws), 1), dtype=torch.int32, device=bufs.dev_status.device)
    out = bufs.out_struct()
    _check(lib().vgx_concave_triangulate_rings(ctx.handle, poly_dev.data_ptr() if ndraws else None, subpaths_dev.data_ptr() if ndraws else None,
                                               draw_info_dev.data_ptr() if ndraws else None, draws_dev.data_ptr() if ndraws else None, int(ndraws), C.byref(out),
                                               draw_route.data_ptr(), bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_concave_triangulate_rings")
    return draw_route


def concave_triangulate_nested(ctx, poly_dev, subpaths_dev, draw_info_dev, draws_dev, ndraws, bufs, draw_route=None):
    """concave_triangulate_rings() that also triangulates several outlines in one path and islands inside holes: the rings are cut by
    containment depth into groups of one outer ring with its holes, each triangulated by the rings rule
    (vgx_concave_triangulate_nested in include/vgx.h). A draw of one group gets concave_triangulate_rings()' bytes."""
    import torch
    if draw_route is None:
        draw_route = torch.zeros(max(int(ndraws), 1), dtype=torch.int32, device=bufs.dev_status.device)
    out = bufs.out_struct()
    _check(lib().vgx_concave_triangulate_nested(ctx.handle, poly_dev.data_ptr() if ndraws else None, subpaths_dev.data_ptr() if ndraws else None,
                                                draw_info_dev.data_ptr() if ndraws else None, draws_dev.data_ptr() if ndraws else None, int(ndraws), C.byref(out),
                                                draw_route.data_ptr(), bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_concave_triangulate_nested")
    return draw_route


# ---- text runs (vgx_text_quads): glyph layout and the atlas stay with the caller -------------------------------------
def text_runs_dense(runs, first_vertex=0, first_index=0):
    """The dense layout for a vgx_text_run array (capi.text_run_dtype, first_quad / num_quads set): every run's vertices and
    indices directly behind its predecessor's, the first at (first_vertex, first_index). With runs that cover the quads
    without gaps from quad 0 this is first_vertex = 4 * first_quad, first_index = 6 * first_quad. In place; returns
    (vertices, indices) = the end of the last run."""
    import numpy as np
    n = runs["num_quads"].astype(np.uint64)
    before = np.cumsum(n) - n
    runs["first_vertex"] = np.uint64(first_vertex) + np.uint64(4) * before
    runs["first_index"] = np.uint64(first_index) + np.uint64(6) * before
    total = int(n.sum())
    return int(first_vertex) + 4 * total, int(first_index) + 6 * total


def text_quads(ctx, quads_dev, nquads, runs_dev, nruns, bufs, first_mesh=0, uv_dev=None, uv_bytes=0):
    """One mesh per run at the run's places in `bufs` (see include/vgx.h). quads_dev: float32 [nquads, 8] device tensor
    (FONSquad), runs_dev: uint8 device tensor of 80-byte vgx_text_run records, uv_dev: the UV stream ([cap_vertices] x
    uv_bytes) or None. Asynchronous; totals / status land in bufs.dev_*."""
    out = bufs.out_struct()
    _check(lib().vgx_text_quads(ctx.handle, quads_dev.data_ptr() if nquads else None, nquads, runs_dev.data_ptr() if nruns else None, nruns,
                                first_mesh, C.byref(out), uv_dev.data_ptr() if uv_dev is not None else None, uv_bytes if uv_dev is not None else 0,
                                bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_text_quads")


# ---- merging external meshes into a frame (vgx_merge) ---------------------------------------------------------------
def mesh_seq(bufs, nv, ni, nm):
    """A finished mesh sequence (what vgx_tessellate / vgx_concave_emit wrote into `bufs`) as a vgx_cache_desc."""
    return capi.CacheDesc(bufs.pos.data_ptr(), bufs.color.data_ptr(), bufs.idx.data_ptr(), bufs.meshes.data_ptr(), int(nm), int(nv), int(ni))


def merge(ctx, seq_a, seq_b, b_draw_dev, draws_dev, ndraws, bufs, b_uv_dev=None):
    """Both sequences interleaved by draw index into `bufs` (honours an armed assembly). b_draw_dev: int32 device tensor, the
    frame draw of every mesh of seq_b (or None). b_uv_dev: per-vertex UVs of seq_b (IndexedTriList meshes), copied into the
    armed assembly's UV stream. Asynchronous; totals / status land in bufs.dev_*."""
    out = bufs.out_struct()
    _check(lib().vgx_merge_uv(ctx.handle, C.byref(seq_a), C.byref(seq_b), b_draw_dev.data_ptr() if b_draw_dev is not None else None,
                              b_uv_dev.data_ptr() if b_uv_dev is not None else None,
                              draws_dev.data_ptr() if draws_dev is not None else None, ndraws, C.byref(out),
                              bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_merge_uv")


def merge_uv_stream(ctx, seq_a, seq_b, b_draw_dev, b_uv_dev, uv_bytes, draws_dev, ndraws, bufs, out_uv_dev):
    """merge() with a UV stream of the caller's: b_uv_dev (uv_bytes per vertex of seq_b, 4 or 8) lands in out_uv_dev ([capacity of
    bufs in vertices] x uv_bytes) at the merged places of seq_b's vertices; out_uv_dev is written nowhere else, and an armed
    assembly's own UV stream is left alone. What raster_textured() reads. Asynchronous; totals / status land in bufs.dev_*."""
    out = bufs.out_struct()
    _check(lib().vgx_merge_uv_stream(ctx.handle, C.byref(seq_a), C.byref(seq_b), b_draw_dev.data_ptr() if b_draw_dev is not None else None,
                                     b_uv_dev.data_ptr(), int(uv_bytes), draws_dev.data_ptr() if draws_dev is not None else None, ndraws, C.byref(out),
                                     out_uv_dev.data_ptr(), bufs.dev_sizes.data_ptr(), bufs.dev_status.data_ptr(), _stream_ptr()), "vgx_merge_uv_stream")
