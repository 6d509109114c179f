"""GPU: vgx_concave_contours (csrc/vgx_concave.hip: k_concave_contours behind the size scan) against its lane code on the inputs
tests/test_concave_contours_cpu.py takes -- every byte of the four streams --, the capacities with guard regions, VGX_E_MESH_TOO_LARGE, and
against the two older device calls: the fringe mesh equals vgx_concave_emit with zero tess input, the moved vertices equal
vgx_concave_move, for the same contours."""
import ctypes as C

import numpy as np
import pytest

import raster_harness as H
import raster_model as R
import test_gpu_concave as TC
from raster_harness import host, rt, to_dev  # noqa: F401 (host, rt: fixtures)

pytestmark = pytest.mark.gpu
capi = R.capi
F = np.float32
GUARD = H.OUT_GUARD


class DevOut:
    """Out of tests/raster_harness.py in device memory: the streams between guard regions."""

    def __init__(self, cap_v, cap_i, cap_m, pad=64):
        import torch
        self.caps, self.pad = (cap_v, cap_i, cap_m), pad
        self.sizes = [8 * (cap_v + 2 * pad), 4 * (cap_v + 2 * pad), 2 * (cap_i + 2 * pad), 32 * (cap_m + 2 * pad)]
        self.t = [torch.full((n,), GUARD, dtype=torch.uint8, device="cuda:0") for n in self.sizes]
        self.struct = capi.MeshOut(*[t.data_ptr() + pad * w for t, w in zip(self.t, (8, 4, 2, 32))], cap_v, cap_i, cap_m)
        self.dev_sizes = torch.zeros(10, dtype=torch.int64, device="cuda:0")
        self.dev_status = torch.full((1,), 77, dtype=torch.int32, device="cuda:0")

    def raw(self):
        return [t.cpu().numpy() for t in self.t]


def gpu_contours(rt, ctx, fl, out):
    import torch
    d = [to_dev(a) for a in (fl.poly, fl.subs, fl.info, fl.draws)]
    rc = rt.lib().vgx_concave_contours(ctx.handle, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(fl.specs), C.byref(out.struct),
                                       out.dev_sizes.data_ptr(), out.dev_status.data_ptr(), rt._stream_ptr())
    torch.cuda.synchronize()
    assert rc == capi.VGX_OK
    s = out.dev_sizes.cpu().numpy()
    return int(out.dev_status.item()), (int(s[2]), int(s[3]), int(s[4]))


def same_bytes(out, hout):
    """Every byte of the four buffers, guard regions included; the mesh records' bytes past the meshes written are guards on both."""
    return all(np.array_equal(a, b.reshape(-1)) for a, b in zip(out.raw(), hout.raw))


def test_kernel_equals_lane_code(rt, gpu_ctx, host):
    fl = H.Flat(H.contour_specs())
    nm, nv, ni = fl.expected_sizes()
    for caps in ((nv, ni, nm), (nv + 5, ni + 3, nm + 2)):
        out, hout = DevOut(*caps), H.Out(*caps)
        st, sizes = gpu_contours(rt, gpu_ctx, fl, out)
        assert (st, sizes) == H.host_contours(host, fl, hout) == (capi.VGX_OK, (nm, nv, ni))
        assert same_bytes(out, hout)
    H.check_structure(fl, *hout.streams(nm, nv, ni))


@pytest.mark.parametrize("short", ["vertices", "indices", "meshes"])
def test_nospace_writes_nothing_past_a_capacity(rt, gpu_ctx, host, short):
    fl = H.Flat(H.contour_specs())
    nm, nv, ni = fl.expected_sizes()
    caps = (nv - (short == "vertices"), ni - (short == "indices"), nm - (short == "meshes"))
    out, hout = DevOut(*caps), H.Out(*caps)
    st, sizes = gpu_contours(rt, gpu_ctx, fl, out)
    assert st == capi.VGX_E_NOSPACE and sizes == (nm, nv, ni)
    assert H.host_contours(host, fl, hout) == (st, sizes) and same_bytes(out, hout)
    assert all((r == GUARD).all() for r in out.raw()[:3])


def test_mesh_too_large_and_misaligned_output(rt, gpu_ctx):
    for n, want in ((32768, capi.VGX_OK), (32769, capi.VGX_E_MESH_TOO_LARGE)):
        fl = H.Flat([([TC._ring(0, 0, 1000, n)], H.CONCAVE | H.AA, 0xFFFFFFFF, 1.0)])
        nm, nv, ni = fl.expected_sizes()
        out = DevOut(nv, ni, nm)
        st, _ = gpu_contours(rt, gpu_ctx, fl, out)
        assert st == want and (want == capi.VGX_OK or all((r == GUARD).all() for r in out.raw()[:3]))
    fl = H.Flat(H.contour_specs())
    nm, nv, ni = fl.expected_sizes()
    d = [to_dev(a) for a in (fl.poly, fl.subs, fl.info, fl.draws)]
    for k, off in enumerate((4, 2, 1, 4)):
        out = DevOut(nv, ni, nm)
        ptrs = [getattr(out.struct, n) for n in ("pos", "color", "idx", "meshes")]
        ptrs[k] += off
        bad = capi.MeshOut(*ptrs, nv, ni, nm)
        assert rt.lib().vgx_concave_contours(gpu_ctx.handle, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(fl.specs), C.byref(bad),
                                             out.dev_sizes.data_ptr(), out.dev_status.data_ptr(), rt._stream_ptr()) == capi.VGX_E_INVALID_ARG


def test_fringe_equals_concave_emit_and_moved_equals_concave_move(rt, gpu_ctx):
    """The draw's own sub-paths as the boundary contours of vgx_concave_move / vgx_concave_emit (zero tess input)."""
    import torch
    specs = [s for s in H.contour_specs() if s[1] & H.AA and s[1] & H.CONCAVE and len(s[0])]
    fl = H.Flat(specs)
    nm, nv, ni = fl.expected_sizes()
    out = DevOut(nv, ni, nm)
    assert gpu_contours(rt, gpu_ctx, fl, out)[0] == capi.VGX_OK
    raw = out.raw()
    p = out.pad
    pos, col = raw[0].view(F).reshape(-1, 2)[p:p + nv], raw[1].view(np.uint32)[p:p + nv]
    idx, meshes = raw[2].view(np.uint16)[p:p + ni], raw[3].view(capi.mesh_dtype)[p:p + nm]
    cont, fills = [], np.zeros(len(specs), dtype=capi.concave_fill_dtype)
    at = 0
    for k, (contours, _, color, fringe) in enumerate(specs):
        fills[k]["first_contour"], fills[k]["num_contours"], fills[k]["color"], fills[k]["fringe"] = len(cont), len(contours), color, fringe
        for c in contours:
            cont.append((at, len(c), k))
            at += len(c)
    cont = np.array(cont, dtype=capi.contour_dtype)
    verts = torch.from_numpy(fl.poly).to("cuda:0")
    cd, fd = to_dev(cont), to_dev(fills)
    moved = rt.concave_move(gpu_ctx, verts, cd, len(cont), fd, len(specs)).cpu().numpy()
    V = at
    B = rt.MeshBuffers(verts.device, 2 * V, 6 * V, len(specs))
    one = torch.zeros(2, dtype=torch.float32, device="cuda:0")
    rt.concave_emit(gpu_ctx, verts, cd, len(cont), fd, len(specs), one, one.view(torch.int16), B)
    torch.cuda.synchronize()
    assert int(B.dev_status.item()) == capi.VGX_OK
    epos, ecol = B.pos[:2 * V].cpu().numpy(), B.color[:2 * V].cpu().numpy().view(np.uint32)
    eidx, em = B.idx[:6 * V].cpu().numpy().view(np.uint16), B.meshes[:len(specs) * 32].cpu().numpy().view(capi.mesh_dtype)
    at = 0
    for k in range(len(specs)):
        fr, it = meshes[2 * k], meshes[2 * k + 1]
        e = em[k]
        n2, n6 = int(e["num_vertices"]), int(e["num_indices"])
        assert (int(fr["num_vertices"]), int(fr["num_indices"]), int(fr["subpath_kind"])) == (n2, n6, int(e["subpath_kind"]))
        a, b = int(fr["first_vertex"]), int(e["first_vertex"])
        assert np.array_equal(pos[a:a + n2].view(np.uint32), epos[b:b + n2].view(np.uint32)) and np.array_equal(col[a:a + n2], ecol[b:b + n2])
        assert np.array_equal(idx[int(fr["first_index"]):int(fr["first_index"]) + n6], eidx[int(e["first_index"]):int(e["first_index"]) + n6])
        a, n = int(it["first_vertex"]), int(it["num_vertices"])
        assert n == n2 // 2 and np.array_equal(pos[a:a + n].view(np.uint32), moved[at:at + n].view(np.uint32))
        at += n
