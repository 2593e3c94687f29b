"""The initial guess by restriction, as the reference states it (buildVelocityMappingPartial, cpp:2291-2402): a FIFO queue of
(face, fp32 weight, level).  Popping a level-0 entry adds weight * velocity[face] to a double; popping any other entry pushes its
3 x 4 finer faces -- child 0..3 (getChildFace), and for each child the in-axis offsets -1, 0, +1 -- with the weight
(float)(rw * (double)w), rw = 1/16, 1/8, 1/16.  Every entry of one level leaves the queue before any entry of the next, so the queue
is expanded here one whole level at a time, in NumPy; the leaves then stand in the order they are popped, and the sum is taken strictly
left to right (np.add.accumulate, which cannot re-associate, not np.sum).  Leaves beyond the velocity lattice are read with clamped
coordinates (the reference reads out of bounds there; both implementations clamp).

This file shares no code with the oracle's depth-first recursion (restrict_rec) or with the kernels' mixed-radix digits.  A level-l row has
12^l leaves: the model is used up to MAX_LEVEL.

The keyword switches state WRONG restrictions on purpose (tests show that the cases can tell them apart): reverse folds right to left,
round_weights=False multiplies the weights in double without the fp32 rounding per level, clamp=False reads 0 beyond the lattice.
"""
import numpy as np

IN_AXIS = (1.0 / 16.0, 1.0 / 8.0, 1.0 / 16.0)
MAX_LEVEL = 5
CHUNK = 1 << 22          # leaves expanded at a time


def expand(faces, weights, axis):
    """one level of the queue: faces [n, 3] (i, j, k), weights [n] -> 12 n entries in push order"""
    n = len(faces)
    u, v = (axis + 1) % 3, (axis + 2) % 3
    out = np.repeat(2 * faces, 12, axis=0).reshape(n, 4, 3, 3)
    for child in range(4):
        out[:, child, :, u] += child & 1
        out[:, child, :, v] += (child >> 1) & 1
    for o in range(3):
        out[:, :, o, axis] += o - 1
    rw = np.asarray(IN_AXIS, np.float64)
    w = rw[None, None, :] * weights.astype(np.float64)[:, None, None]          # restrictionWeight * localWeight, in double
    w = np.broadcast_to(w, (n, 4, 3))
    if weights.dtype == np.float32:
        w = w.astype(np.float32)                                               # stored in fpreal32 myWeight
    return out.reshape(12 * n, 3), np.ascontiguousarray(w).reshape(12 * n)


def restrict(velocity, faces, axis, level, *, reverse=False, round_weights=True, clamp=True):
    """restricted velocity (float64 [n]) of the level-`level` faces [n, 3] of `axis`; velocity: the fp32 face lattice [z, y, x] of `axis`"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    vel = np.asarray(velocity, np.float32)
    shape = np.asarray(vel.shape[::-1], np.int64)
    per = 12 ** level
    out = np.empty(len(faces), np.float64)
    step = max(1, CHUNK // per)
    for lo in range(0, len(faces), step):
        f = faces[lo:lo + step]
        w = np.ones(len(f), np.float32 if round_weights else np.float64)
        for _ in range(level):
            f, w = expand(f, w, axis)
        if clamp:
            q = np.clip(f, 0, shape - 1)
            val = vel[q[:, 2], q[:, 1], q[:, 0]]
        else:
            inside = ((f >= 0) & (f < shape)).all(axis=1)
            q = np.where(inside[:, None], f, 0)
            val = np.where(inside, vel[q[:, 2], q[:, 1], q[:, 0]], np.float32(0))
        terms = (w.astype(np.float64) * val.astype(np.float64)).reshape(-1, per)
        if reverse:
            terms = terms[:, ::-1]
        out[lo:lo + step] = np.add.accumulate(terms, axis=1)[:, -1]
    return out


def initial_guess(vidx, velocity, n_velocity, f32=False, max_level=MAX_LEVEL, **wrong):
    """x0 of a velocity index pyramid (vidx[l][a] int32 [z, y, x]); rows of a level above max_level are NaN.  f32: the initial guess is a
    float vector (SolveType = fpreal32)."""
    x0 = np.full(n_velocity, np.nan)
    for l, per_level in enumerate(vidx):
        if l > max_level:
            break
        for a, lat in enumerate(per_level):
            kji = np.argwhere(lat >= 0)
            if len(kji):
                x0[lat[lat >= 0]] = restrict(velocity[a], kji[:, ::-1], a, l, **wrong)
    return x0.astype(np.float32).astype(np.float64) if f32 else x0
