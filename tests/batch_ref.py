"""The orientation map of srcnn_gather_batch restated in numpy.

A record's `op` is an element of the dihedral group of the square, three bits:
bit 1 mirrors the footprint's rows, bit 0 its columns, bit 2 transposes
afterwards.  The output tile is tw x th (th rows of tw floats); its source
footprint is sw x sh = tw x th, swapped when bit 2 is set."""
import numpy as np

OPS = tuple(range(8))


def footprint(tw, th, op):
    """(sw, sh): the extent of the source footprint of a tw x th tile."""
    return (th, tw) if op & 4 else (tw, th)


def orient(foot, op):
    """The tile a footprint [sh][sw] leaves as."""
    a = np.asarray(foot)
    assert a.ndim == 2 and 0 <= op <= 7
    if op & 2:
        a = a[::-1, :]
    if op & 1:
        a = a[:, ::-1]
    if op & 4:
        a = a.T
    return np.ascontiguousarray(a)


def orient_by_index(foot, op):
    """The same map spelt out element by element, as the spec words it."""
    foot = np.asarray(foot)
    sh, sw = foot.shape
    tw, th = (sh, sw) if op & 4 else (sw, sh)
    out = np.empty((th, tw), foot.dtype)
    for r in range(th):
        for c in range(tw):
            a, b = (c, r) if op & 4 else (r, c)
            if op & 2:
                a = sh - 1 - a
            if op & 1:
                b = sw - 1 - b
            out[r, c] = foot[a, b]
    return out


def window(plane, x, y, tw, th, op):
    """The footprint of a tw x th tile with orientation `op` at (x, y) of a 2-D plane."""
    sw, sh = footprint(tw, th, op)
    assert x + sw <= plane.shape[1] and y + sh <= plane.shape[0]
    return plane[y:y + sh, x:x + sw]
