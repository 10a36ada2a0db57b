"""NumPy statement of pd_pose_chain (include/polardepth.h): the matching-pose half of the reference's predict_poses
(trainer.py:708-746) for one direction.  The fp32 link matrices are tests/pose_ref.pose_matrix rounded once; the chain
product is formed in fp64 from fp32 values, term by term in the stated order (NumPy fuses nothing), and rounded once.
Test infrastructure only."""
import numpy as np

import pose_ref

F64, F32 = np.float64, np.float32
MAX_LINKS = 8


def link_matrices(axisangle, translation, direction):
    """(M, Minv) [L,N,4,4] float32: pd_pose_matrix_fwd of every link with invert = (direction < 0), and with it flipped."""
    aa = np.asarray(axisangle, F32)
    L, N = aa.shape[:2]
    tr = np.asarray(translation, F32)
    inv = direction < 0
    with np.errstate(all="ignore"):
        M = pose_ref.pose_matrix(aa.reshape(L * N, 3), tr.reshape(L * N, 3), inv).astype(F32).reshape(L, N, 4, 4)
        Mi = pose_ref.pose_matrix(aa.reshape(L * N, 3), tr.reshape(L * N, 3), not inv).astype(F32).reshape(L, N, 4, 4)
    return M, Mi


def chain_product(M, A):
    """[N,4,4] float32 = M A per item: ((m_i0 a_0c + m_i1 a_1c) + m_i2 a_2c) + m_i3 a_3c in fp64, rounded once."""
    m, a = np.asarray(M, F32).astype(F64), np.asarray(A, F32).astype(F64)
    out = np.empty(m.shape, F64)
    with np.errstate(all="ignore"):
        for i in range(4):
            for c in range(4):
                out[:, i, c] = ((m[:, i, 0] * a[:, 0, c] + m[:, i, 1] * a[:, 1, c]) + m[:, i, 2] * a[:, 2, c]) + \
                    m[:, i, 3] * a[:, 3, c]
        return out.astype(F32)


def pose_chain(axisangle, translation, present=None, init=None, direction=-1):
    """(rel, rel_inv) [L,N,4,4] float32.  axisangle / translation [L,N,3] (or [L,N,1,3]), present [L,N] or None, init
    [N,4,4] or None, direction -1 or 1."""
    assert direction in (-1, 1)
    aa = np.asarray(axisangle, F32)
    L, N = aa.shape[:2]
    assert 1 <= L <= MAX_LINKS and N >= 1
    M, Mi = link_matrices(aa, translation, direction)
    rel = np.empty((L, N, 4, 4), F32)
    A = None if init is None else np.asarray(init, F32).reshape(N, 4, 4)
    for k in range(L):
        A = M[k].copy() if A is None else chain_product(M[k], A)
        if present is not None:
            A[np.asarray(present, F32)[k] == 0] = F32(0)
        rel[k] = A                                   # the STORED matrix is what the next link multiplies
    return rel, Mi
