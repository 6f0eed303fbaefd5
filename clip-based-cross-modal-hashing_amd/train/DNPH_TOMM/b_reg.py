"""Noise assignment of the DNPH step (reference train/DNPH_TOMM/b_reg.py:5-40).  Upstream solves the Hungarian assignment on
the host (scipy); `assign_noise(..., "gpu")` solves both modalities' problems exactly on the device (csrc/assign.hip) without a
host round trip, `assign_noise(..., "host")` is upstream's path (`gene_noise`).  Both return the same rows unless two different
assignments have exactly the same optimal cost; then each returns an optimum, the device always the same one (its tie rule:
lowest reduced cost, then an unassigned column, then the lowest column index).  Duplicate noise rows are no such case: the
permutations may differ there, the assigned rows do not."""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment


def rand_unit_rect(npoints, ndim):
    vec = np.random.randint(0, 2, size=(npoints, ndim))
    vec[vec == 0] = -1
    return vec


def gene_noise(embeedings, noises):
    """Assign each sample the +-1 noise row that minimises the total L2 cost (float64 like upstream)."""
    e = np.asarray(embeedings, dtype=np.float64)
    nz = np.asarray(noises, dtype=np.float64)
    losses = np.linalg.norm(e[:, None, :] - nz[None, :, :], axis=2)
    row_ind, col_ind = linear_sum_assignment(losses)
    new_noise = np.empty(shape=nz.shape, dtype='float64')
    new_noise[row_ind] = nz[col_ind]
    return new_noise


def assign_noise(hash_img, hash_text, s_vector, how="gpu"):
    """The noise rows of both modalities for one step, as f32 tensors on the hashes' device.  s_vector: the +-1 matrix of
    `rand_unit_rect` (host, the shape of the hashes)."""
    dev = hash_img.device
    if how == "host":
        on_host = lambda h: h.cpu().detach().numpy()
        to_dev = lambda a: torch.from_numpy(a).float().to(dev)
        return to_dev(gene_noise(on_host(hash_img), s_vector)), to_dev(gene_noise(on_host(hash_text), s_vector))
    if how != "gpu":
        raise ValueError(f"assign_noise: how = {how!r}, expected 'gpu' or 'host'")
    import cmh_native as N
    # s_vector does not depend on device data: the upload is queued behind the forward without waiting for it
    rows = torch.from_numpy(np.ascontiguousarray(s_vector, dtype=np.float32)).pin_memory().to(dev, non_blocking=True)
    out = N.assign_rows(torch.stack((hash_img.detach().float(), hash_text.detach().float())), rows)
    return out[0], out[1]
