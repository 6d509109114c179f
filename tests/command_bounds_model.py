"""numpy statement of vgx_command_bounds (include/vgx.h). Not collected by pytest."""
import numpy as np

import raster_commands_model as CM

capi = CM.capi
EMPTY = (np.inf, np.inf, -np.inf, -np.inf)


def valid(sc, c):
    """The record's ranges lie inside the streams and it has at most 65536 vertices; nothing else is examined."""
    r = sc.cmds[c]
    return int(r["num_vertices"]) <= 65536 and int(r["first_vertex"]) + int(r["num_vertices"]) <= sc.nv and int(r["first_index"]) + int(r["num_indices"]) <= sc.ni


def boxes(sc, begin=0, end=0xFFFFFFFF, table=None):
    """(table, status): entries [begin, min(end, real count)) of `table` (float32 [num_cmds, 4], changed in place; None: one of 77.0) set
    to minx, miny, maxx, maxy over the corners of the command's triangles whose indices are all below num_vertices; the others stay."""
    table = np.full((sc.cmds.shape[0], 4), 77.0, dtype=np.float32) if table is None else table
    rng = range(begin, min(end, sc.n))
    for c in rng:
        table[c] = EMPTY
        if valid(sc, c):
            r = sc.cmds[c]
            fi, nv = int(r["first_index"]), int(r["num_vertices"])
            tri = sc.idx[fi:fi + int(r["num_indices"]) // 3 * 3].astype(np.int64).reshape(-1, 3)
            p = sc.pos[int(r["first_vertex"]) + tri[(tri < nv).all(axis=1)].reshape(-1)]
            if p.shape[0]:
                table[c] = (*p.min(axis=0), *p.max(axis=0))
    return table, (capi.VGX_OK if all(valid(sc, c) for c in rng) else capi.VGX_E_INVALID_ARG)
