"""Float64 NumPy restatement of DJSRH's joint-semantics target, loss and hand-derived gradient (csrc/djsrh.hip, train/DJSRH/loss.py;
Su, Zhong, Zhang, ICCV 2019), and the seeded cases the host and GPU tests share.

    n(x) = x / max(|x|, 1e-12) per row
    St = beta (2 n(fi) n(fi)^T - 1) + (1 - beta) (2 n(ft) n(ft)^T - 1),   S = mu ((1 - eta) St + (eta / B) St St^T)
    R_II = b_I b_I^T - S, R_IT = b_I b_T^T - S, R_TT = b_T b_T^T - S with b = n(h)
    loss = lambda1 mean(R_II^2) + mean(R_IT^2) + lambda2 mean(R_TT^2)
    c = 2 dloss / B^2:  g_I = c (2 lambda1 R_II b_I + R_IT b_T),  g_T = c (2 lambda2 R_TT b_T + R_IT^T b_I)
    dh = (g - b (b . g)) / max(|h|, 1e-12) per row"""
import numpy as np

SCALARS = (0.9, 0.4, 1.5, 0.1, 0.1)                                 # beta, eta, mu, lambda1, lambda2: the trainer's defaults
HOST_SHAPES = [(1, 16, 64), (2, 24, 40), (65, 64, 100), (300, 128, 64)]
# one row; ragged K and D; both sides of the 64-row wave and of the 32-row tile edge; the default batch
GPU_SHAPES = [(1, 16, 64), (2, 24, 40), (63, 16, 64), (64, 64, 512), (65, 64, 100), (129, 128, 768), (300, 64, 512)]
EPS = 1e-12


def normalize(x):
    x = np.asarray(x, np.float64)
    n = np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), EPS)
    return x / n, n


def s_tilde(fi, ft, beta):
    a, t = normalize(fi)[0], normalize(ft)[0]
    return beta * (2.0 * (a @ a.T) - 1.0) + (1.0 - beta) * (2.0 * (t @ t.T) - 1.0)


def target(fi, ft, beta, eta, mu):
    st = s_tilde(fi, ft, beta)
    return mu * ((1.0 - eta) * st + (eta / st.shape[0]) * (st @ st.T))


def loss(hi, ht, S, lambda1, lambda2, dloss=1.0):
    """-> dict: loss, terms [3] (II, IT, TT), gi, gt (the gradients towards hi and ht, times dloss)"""
    (bi, ni), (bt, nt) = normalize(hi), normalize(ht)
    S = np.asarray(S, np.float64)
    B = bi.shape[0]
    r_ii, r_it, r_tt = bi @ bi.T - S, bi @ bt.T - S, bt @ bt.T - S
    terms = np.array([(r_ii ** 2).mean(), (r_it ** 2).mean(), (r_tt ** 2).mean()])
    c = 2.0 * dloss / (B * B)
    g_i = c * (2.0 * lambda1 * (r_ii @ bi) + r_it @ bt)
    g_t = c * (2.0 * lambda2 * (r_tt @ bt) + r_it.T @ bi)
    back = lambda g, b, n: (g - b * (b * g).sum(1, keepdims=True)) / n
    return {"loss": lambda1 * terms[0] + terms[1] + lambda2 * terms[2], "terms": terms, "gi": back(g_i, bi, ni), "gt": back(g_t, bt, nt)}


def case(B, K, D, seed=0):
    """f32 arrays: features fi, ft [B, D] that share a latent part (so S has structure), codes hi, ht [B, K] = tanh(randn): no zero row"""
    rng = np.random.default_rng([20191027, B, K, D, seed])
    shared = rng.standard_normal((B, D))
    fi = (shared + 0.7 * rng.standard_normal((B, D)) + 0.3).astype(np.float32)
    ft = (shared @ (rng.standard_normal((D, D)) / np.sqrt(D)) + 0.7 * rng.standard_normal((B, D))).astype(np.float32)
    hi, ht = (np.tanh(rng.standard_normal((B, K))).astype(np.float32) for _ in range(2))
    return {"fi": fi, "ft": ft, "hi": hi, "ht": ht}


def sgd_losses(hi, ht, S, lambda1, lambda2, steps, lr):
    """plain SGD on hi and ht in float64 -> the loss before each step"""
    hi, ht = np.asarray(hi, np.float64).copy(), np.asarray(ht, np.float64).copy()
    out = []
    for _ in range(steps):
        r = loss(hi, ht, S, lambda1, lambda2)
        out.append(r["loss"])
        hi -= lr * r["gi"]
        ht -= lr * r["gt"]
    return np.array(out)
