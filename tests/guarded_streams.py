"""Caller buffers for the entries that write mesh streams, placed where a caller may place them and watched on both sides.

include/vgx.h asks of a vgx_mesh_out the alignment of its element types and no more: pos 8 bytes, color 4, idx 2, the mesh table 8.
GuardedOut hands such buffers over: every stream is a range of a uint8 arena of its own, filled with the stream's byte pattern, with
at least GUARD bytes of pattern in front of the range and behind it, the first byte at a chosen residue modulo 128 (SKEWS: S0 whole
lines, S1 the least each element type allows, S2 the first element the last of a line, S3 in between). It offers what
runtime.MeshBuffers offers, so every wrapper of the runtime takes it unchanged. read() compares all of both guards of every arena
byte by byte before it returns the ranges.

check_guards / place are plain numpy / integer functions: tests/test_guarded_streams_cpu.py pins them without a GPU."""
import importlib

import numpy as np

capi = importlib.import_module("vg-renderer_amd.capi")

GUARD = 4096   # bytes of pattern at least on either side of a range
LINE = 128     # residues are taken modulo this (a cache line of the device)
STREAMS = ("pos", "color", "idx", "meshes", "uv")
ELEM_BYTES = {"pos": 8, "color": 4, "idx": 2, "meshes": 32}
PATTERN = {"pos": 0xA7, "color": 0x3C, "idx": 0x5E, "meshes": 0xE1, "uv": 0x96}  # one byte value per stream, all different
# residues modulo 128 of the first byte of pos, color, idx, the mesh table, and of a UV stream of 4 / of 8 bytes per vertex
SKEWS = {
    "S0": {"pos": 0, "color": 0, "idx": 0, "meshes": 0, "uv4": 0, "uv8": 0},
    "S1": {"pos": 8, "color": 4, "idx": 2, "meshes": 8, "uv4": 4, "uv8": 8},
    "S2": {"pos": 120, "color": 124, "idx": 126, "meshes": 24, "uv4": 124, "uv8": 120},
    "S3": {"pos": 56, "color": 12, "idx": 14, "meshes": 16, "uv4": 12, "uv8": 56},
}
SKEW_NAMES = tuple(SKEWS)


def place(base, residue, guard=GUARD, line=LINE):
    """The offset of a range in an arena that starts at address `base`: the least one >= guard whose address is `residue` mod line."""
    return guard + (residue - (base + guard)) % line


def arena_bytes(nbytes, guard=GUARD, line=LINE):
    """An arena this long holds a range of nbytes at any place() with `guard` bytes behind it."""
    return int(nbytes) + 2 * guard + line


def check_guards(host_bytes, begin, end, pattern, stream="stream"):
    """host_bytes: a uint8 numpy copy of a whole arena whose range is [begin, end). Every byte outside the range must hold `pattern`.
    Raises AssertionError that names the stream, the side ("front" / "behind") and the offset of the first differing byte relative
    to the range: negative in front of it (-1: the byte before the first), from 0 behind it (0: the byte after the last)."""
    host_bytes = np.asarray(host_bytes)
    assert host_bytes.dtype == np.uint8 and host_bytes.ndim == 1 and 0 <= begin <= end <= host_bytes.shape[0]
    front = np.flatnonzero(host_bytes[:begin] != pattern)
    if front.shape[0]:
        at = int(front[0])
        raise AssertionError("%s: front guard touched at offset %d (byte %d of the arena holds 0x%02X, pattern 0x%02X; %d bytes differ)"
                             % (stream, at - begin, at, int(host_bytes[at]), pattern, front.shape[0]))
    behind = np.flatnonzero(host_bytes[end:] != pattern)
    if behind.shape[0]:
        at = int(behind[0])
        raise AssertionError("%s: behind guard touched at offset %d (byte %d of the arena holds 0x%02X, pattern 0x%02X; %d bytes differ)"
                             % (stream, at, end + at, int(host_bytes[end + at]), pattern, behind.shape[0]))


class Result:
    """What read() returns: the fields of util.run_async's result that a buffer can give."""


class GuardedOut:
    """Output buffers of exactly (nv, ni, nm) elements -- and a UV stream of nv x uv_bytes when uv_bytes is 4 or 8 -- between guards,
    at the residues of SKEWS[skew]. Has pos / color / idx / meshes (typed views of the ranges), cap, dev_sizes, dev_status and
    out_struct() like runtime.MeshBuffers; uv is the int16 [nv, 2] or float32 [nv, 2] view of the UV range."""

    def __init__(self, rt, nv, ni, nm, skew, uv_bytes=0, device="cuda:0"):
        import torch
        assert uv_bytes in (0, 4, 8)
        self.rt = rt
        self.cap = (int(nv), int(ni), int(nm))
        self.skew = skew
        self.uv_bytes = uv_bytes
        nbytes = {"pos": 8 * self.cap[0], "color": 4 * self.cap[0], "idx": 2 * self.cap[1], "meshes": 32 * self.cap[2]}
        residue = {k: SKEWS[skew][k] for k in nbytes}
        if uv_bytes:
            nbytes["uv"] = uv_bytes * self.cap[0]
            residue["uv"] = SKEWS[skew]["uv%d" % uv_bytes]
        self.arena, self.begin, self.end = {}, {}, {}
        for k, n in nbytes.items():
            a = torch.full((arena_bytes(n),), PATTERN[k], dtype=torch.uint8, device=device)
            b = place(a.data_ptr(), residue[k])
            assert (a.data_ptr() + b) % LINE == residue[k], (k, skew, a.data_ptr(), b)  # the residue that was reached
            assert b >= GUARD and a.numel() - (b + n) >= GUARD, (k, b, n, a.numel())
            self.arena[k], self.begin[k], self.end[k] = a, b, b + n
        r = {k: self.arena[k][self.begin[k]:self.end[k]] for k in nbytes}
        self.pos = r["pos"].view(torch.float32).view(self.cap[0], 2)
        self.color = r["color"].view(torch.int32)
        self.idx = r["idx"].view(torch.int16)
        self.meshes = r["meshes"]
        self.uv = r["uv"].view(torch.int16 if uv_bytes == 4 else torch.float32).view(self.cap[0], 2) if uv_bytes else None
        self.dev_sizes = torch.zeros(10, dtype=torch.int64, device=device)
        self.dev_status = torch.zeros(1, dtype=torch.int32, device=device)

    def address(self, k):
        """Of the first byte of stream k's range (taken from the arena: a view of no elements need not have one)."""
        return self.arena[k].data_ptr() + self.begin[k]

    def out_struct(self):
        return capi.MeshOut(self.address("pos"), self.address("color"), self.address("idx"), self.address("meshes"), *self.cap)

    def host_arenas(self):
        import torch
        torch.cuda.synchronize()
        return {k: a.cpu().numpy() for k, a in self.arena.items()}

    def read(self):
        """Synchronises; asserts that all of both guards of every arena hold their pattern; returns the ranges: pos float32 [nv, 2],
        color uint32, idx uint16, meshes as capi.mesh_dtype records, uv as uint32 words [nv, uv_bytes / 4] (or None), status,
        dev_sizes (by name) and sizes (the element counts the buffers were made for)."""
        host = self.host_arenas()
        for k, h in host.items():
            check_guards(h, self.begin[k], self.end[k], PATTERN[k], stream="%s (%s)" % (k, self.skew))
        part = {k: h[self.begin[k]:self.end[k]].copy() for k, h in host.items()}
        g = Result()
        g.pos = part["pos"].view(np.float32).reshape(-1, 2)
        g.color = part["color"].view(np.uint32)
        g.idx = part["idx"].view(np.uint16)
        g.meshes = part["meshes"].view(capi.mesh_dtype)
        g.uv = part["uv"].view(np.uint32).reshape(self.cap[0], self.uv_bytes // 4) if self.uv_bytes else None
        g.status = int(self.dev_status.item())
        dev = self.dev_sizes.cpu().numpy()
        g.dev_sizes = {k: int(dev[i]) for i, (k, _) in enumerate(capi.Sizes._fields_)}
        g.sizes = {"num_vertices": self.cap[0], "num_indices": self.cap[1], "num_meshes": self.cap[2]}
        return g

    def assert_untouched(self):
        """Every byte of every arena, the ranges included, still holds its pattern: the call wrote nothing at all."""
        for k, h in self.host_arenas().items():
            check_guards(h, h.shape[0], h.shape[0], PATTERN[k], stream="%s (%s, whole arena)" % (k, self.skew))
