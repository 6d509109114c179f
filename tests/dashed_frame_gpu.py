"""Shared by tests/test_gpu_dashed_frame.py: running vgx_tessellate_dashed, and the COMPOSITION of the entries that existed before it
for the same frame -- tessellate_immediate with the strokes of the dashed draws off (sequence A); flatten -> subpath_draws -> dash ->
stroke_count / stroke_emit restricted to the dashed, stroke-enabled draws (sequence B); vgx_merge."""
import numpy as np

import dashed_frame_model as DM

capi = DM.capi


class Got:
    pass


def upload(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def sizes_of(t):
    z = t.cpu().numpy()
    return {k: int(z[i]) for i, (k, _) in enumerate(capi.Sizes._fields_)}


def read(bufs, sizes):
    g = Got()
    nv, ni, nm = sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"]
    g.pos = bufs.pos[:nv].cpu().numpy()
    g.color = bufs.color[:nv].cpu().numpy().view(np.uint32)
    g.idx = bufs.idx[:ni].cpu().numpy().view(np.uint16)
    g.meshes = bufs.meshes[:nm * 32].cpu().numpy().view(capi.mesh_dtype)
    g.sizes = sizes
    g.bufs = bufs
    return g


def dashed(rt, ctx, pset, dd, n, dashes, pattern, bufs=None, max_calls=4):
    """tessellate_dashed until VGX_OK: the frame (numpy), .statuses, .sizes, .dash_sizes."""
    r = rt.tessellate_dashed(ctx, pset, dd, n, upload(dashes) if dashes is not None else None, upload(np.asarray(pattern, np.float32)), len(pattern), bufs=bufs, max_calls=max_calls)
    return r


def compose(rt, ctx, pset, d, dashes, pattern, assembly=None):
    """The frame from the entries that existed before vgx_tessellate_dashed. assembly: None, or a function arming the context's
    assembly for the merge (A and B are built disarmed: vgx_merge takes mesh-local indices)."""
    import torch
    n = d.shape[0]
    mask = DM.dashed_mask(d, dashes)
    da = d.copy()
    da["stroke_flags"][mask] = 0
    dda = rt.upload_draws(da)
    ia, abufs = rt.tessellate_grow(ctx, pset, dda, n, max_calls=4)
    sa = ia.sizes
    sel = np.flatnonzero(mask)
    if sel.shape[0]:
        ds = d[sel].copy()
        ds["fill_flags"] = 0
        dds = rt.upload_draws(ds)
        flat = rt.flatten(ctx, pset, dds, sel.shape[0], apply_transform=True)
        nsub = flat.sizes["num_subpaths"]
        sd = rt.subpath_draws(ctx, flat.dinfo_dev, sel.shape[0], nsub)
        pat = np.asarray(pattern, np.float32)
        pcs = rt.dash(ctx, flat.poly_dev, flat.subs_dev, sd, nsub, upload(dashes[sel]), sel.shape[0], upload(pat), pat.shape[0])
        npieces = pcs.sizes["num_subpaths"]
        mesh = rt.stroke(ctx, pcs.poly_dev, pcs.subs_dev, pcs.sub_draw_dev, npieces, dds, sel.shape[0], to_host=True)
        assert mesh.sizes["num_meshes"] == npieces  # (every piece has >= 2 vertices)
        b_draw = sel[pcs.sub_draw].astype(np.int32)
        b_sub = (pcs.sub_src.astype(np.int64) - flat.draw_info["first_subpath"][pcs.sub_draw].astype(np.int64)).astype(np.uint32)
        sb, bbufs = mesh.sizes, mesh.bufs
        dash_sizes = (npieces, pcs.sizes["num_poly_vertices"])
    else:
        sb, bbufs = {"num_vertices": 0, "num_indices": 0, "num_meshes": 0}, rt.MeshBuffers("cuda", 1, 1, 1)
        b_draw, b_sub, dash_sizes = np.zeros(0, np.int32), np.zeros(0, np.uint32), (0, 0)
    out = rt.MeshBuffers("cuda", sa["num_vertices"] + sb["num_vertices"], sa["num_indices"] + sb["num_indices"], sa["num_meshes"] + sb["num_meshes"])
    dd = rt.upload_draws(d)
    if assembly:
        assembly(True)
    rt.merge(ctx, rt.mesh_seq(abufs, sa["num_vertices"], sa["num_indices"], sa["num_meshes"]), rt.mesh_seq(bbufs, sb["num_vertices"], sb["num_indices"], sb["num_meshes"]),
             torch.from_numpy(b_draw).cuda() if b_draw.shape[0] else torch.zeros(1, dtype=torch.int32, device="cuda"), dd, n, out)
    torch.cuda.synchronize()
    if assembly:
        assembly(False)
    status = int(out.dev_status.item())
    if assembly and status != 0:  # (the armed assembly's verdict, e.g. VGX_E_MESH_TOO_LARGE: the caller compares it)
        g = Got()
        g.status = status
        return g
    assert status == 0, status
    z = sizes_of(out.dev_sizes)
    g = read(out, z)
    g.status = 0
    # vgx_merge keeps B's sub-path word (the piece's number among the call's lists); the frame call names the SOURCE sub-path
    from_b = ((g.meshes["subpath_kind"] >> 28) >= capi.MESH_STROKE) & mask[g.meshes["draw"]]
    assert int(from_b.sum()) == b_sub.shape[0]
    g.meshes = g.meshes.copy()
    g.meshes["subpath_kind"][from_b] = (g.meshes["subpath_kind"][from_b] & 0xF0000000) | (b_sub & 0x0FFFFFFF)
    g.dash_sizes = dash_sizes
    g.flat_sizes = {k: sa[k] for k in ("num_poly_vertices", "num_subpaths", "num_cmd_instances")}
    return g
