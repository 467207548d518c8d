"""A direct NumPy restatement of the reference's VisualPoseEvidence operator
(backend/operators/visual_pose_evidence.py:261-436), in the reference's own naive N x K einsum form
with np.linalg.svd. It does not use the collapsed sums of the device kernels (gc_vpe.hip), so the
two are independent routes to the same numbers.

The reference ships no test vectors for this operator: parity is pinned by this restatement
("parity unpinned" against reference outputs), as the association's is by oracle/gc_oracle.py.

    measurement means / directions / kappas   structures/measurement_batch.py:389-411
    translation WLS                           visual_pose_evidence.py:74-162
    vMF scatter rotation                      visual_pose_evidence.py:165-253
    operator, empty branch, 22-D embedding    visual_pose_evidence.py:261-436
"""

import numpy as np

from oracle import gc_oracle as O

D_Z = 22


def measurement_means(meas, eps_lift=O.EPS_LIFT, eps_mass=O.EPS_MASS):
    """measurement_batch.py:389-411: positions solve(Λ + εI, θ), directions Ση / (‖Ση‖ + ε), κ = ‖Ση‖,
    and the lifted precisions the operator uses (visual_pose_evidence.py:337)."""
    Lr = np.asarray(meas["Lambdas"], np.float64) + eps_lift * np.eye(3)[None]
    pos = np.linalg.solve(Lr, np.asarray(meas["thetas"], np.float64)[..., None])[..., 0]
    es = np.asarray(meas["etas"], np.float64).sum(axis=1)
    kap = np.linalg.norm(es, axis=1)
    return pos, es / (kap[:, None] + eps_mass), kap, Lr


def translation_wls(mpos, mprec, vpos, pi, idx, R, t, eps_lift):
    """visual_pose_evidence.py:108-148 (the gather clamps its indices, as a JAX gather does)."""
    world = np.einsum("ij,nj->ni", R, mpos)
    cand = vpos[np.clip(idx, 0, vpos.shape[0] - 1)]                      # (N, K, 3)
    resid = cand - world[:, None, :] - t[None, None, :]
    L = np.einsum("n,nij->ij", pi.sum(axis=1), mprec)
    target = cand - world[:, None, :]
    h = np.einsum("nij,nj->i", mprec, np.einsum("nk,nkj->nj", pi, target))
    Lr = np.einsum("nij,nkj->nki", mprec, resid)
    cost = float(np.sum(pi * np.einsum("nki,nki->nk", resid, Lr)))
    return L + eps_lift * np.eye(3), h, cost


def rotation_vmf(mdir, mkap, vdir, vkap, pi, idx, R, eps_lift):
    """visual_pose_evidence.py:200-240. Also returns the scatter S, Σw, R_scatter and the tangent step."""
    j = np.clip(idx, 0, vdir.shape[0] - 1)
    d, km = vdir[j], vkap[j]
    w = pi * np.sqrt(mkap[:, None] * km + 1e-12)
    S = np.einsum("nk,nki,nj->ij", w, d, mdir)
    dots = np.einsum("ni,nki->nk", np.einsum("ij,nj->ni", R, mdir), d)
    cost = float(np.sum(w * (1.0 - dots)))
    U, s, Vt = np.linalg.svd(S)
    L = np.diag(s + eps_lift)
    Rs = U @ Vt
    if np.linalg.det(Rs) < 0:
        Rs = U @ np.diag([1.0, 1.0, -1.0]) @ Vt
    rv = O.so3_log(Rs @ R.T)
    return L, L @ rv, cost, dict(S=S, W=float(w.sum()), sing=s, R_scatter=Rs, rotvec_delta=rv,
                                 reflected=bool(np.linalg.det(U @ Vt) < 0))


def visual_pose_evidence(assoc, meas, view, pose6, eps_lift=O.EPS_LIFT, eps_mass=O.EPS_MASS):
    """visual_pose_evidence.py:261-436 for one linearisation pose [t, rotvec]. assoc: responsibilities,
    candidate_pool_indices, row_masses; meas: Lambdas, thetas, etas, valid_mask; view: positions,
    directions, kappas, valid_mask. Returns the result fields, the certificate scalars and the
    rotation diagnostics as one dict."""
    valid = np.asarray(meas["valid_mask"], bool).reshape(-1)
    pi_all = np.asarray(assoc["responsibilities"], np.float64)
    K = pi_all.shape[1]
    n_valid = int(valid.sum())
    if n_valid == 0 or pi_all.shape[0] == 0 or int(np.asarray(view["valid_mask"]).astype(bool).sum()) == 0:  # :297-318
        return dict(L_pose=eps_lift * np.eye(D_Z), h_pose=np.zeros(D_Z), L_trans=np.zeros((3, 3)), h_trans=np.zeros(3),
                    L_rot=np.zeros((3, 3)), h_rot=np.zeros(3), cost_trans=0.0, cost_rot=0.0, total_weighted_cost=0.0,
                    n_associations=0, mean_transported_mass=0.0, sum_row_masses=0.0, empty=True)
    pose6 = np.asarray(pose6, np.float64).ravel()[:6]
    t, R = pose6[:3], O.so3_exp(pose6[3:6])
    pos, dirs, kap, prec = measurement_means(meas, eps_lift, eps_mass)
    vi = np.where(valid)[0]                                              # :339-351
    pi = pi_all[vi]
    idx = np.asarray(assoc["candidate_pool_indices"])[vi].astype(np.int32)
    rowm = np.asarray(assoc["row_masses"], np.float64)[vi]
    Lt, ht, ct = translation_wls(pos[vi], prec[vi], np.asarray(view["positions"]), pi, idx, R, t, eps_lift)
    Lr, hr, cr, diag = rotation_vmf(dirs[vi], kap[vi], np.asarray(view["directions"]), np.asarray(view["kappas"]), pi,
                                    idx, R, eps_lift)
    L_pose = eps_lift * np.eye(D_Z)                                      # :386-395
    h_pose = np.zeros(D_Z)
    L_pose[0:3, 0:3], h_pose[0:3] = Lt, ht
    L_pose[3:6, 3:6], h_pose[3:6] = Lr, hr
    return dict(L_pose=L_pose, h_pose=h_pose, L_trans=Lt, h_trans=ht, L_rot=Lr, h_rot=hr, cost_trans=ct, cost_rot=cr,
                total_weighted_cost=ct + cr, n_associations=int(pi.shape[0] * K),
                mean_transported_mass=float(np.mean(rowm)), sum_row_masses=float(np.sum(rowm)), empty=False, **diag)
