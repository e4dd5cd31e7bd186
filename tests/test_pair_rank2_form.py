"""The algebra behind csrc/sfmba_device.h pair_product_ab, in numpy: one pair's 6x6 update G_a^T N G_b (G = [-[X]x | I],
N = P_a^T M P_b, P = [[1, 0, -x], [0, 1, -y]]) equals the rank-2 form alpha V_0^T + beta V_1^T with V_r = [X_b x u_r | u_r],
u_r = row r of M P_b, and the coefficients (alpha_i, beta_i) the kernel uses -- the same formulas, in the kernel's row pairing."""
import numpy as np


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def test_rank2_form_is_the_factored_pair_product():
    rng = np.random.default_rng(7)
    for _ in range(20):
        Xa, Xb = rng.normal(size=3), rng.normal(size=3)
        xa, ya, xb, yb = rng.normal(size=4)
        M = rng.normal(size=(2, 2))
        Pa = np.array([[1.0, 0.0, -xa], [0.0, 1.0, -ya]])
        Pb = np.array([[1.0, 0.0, -xb], [0.0, 1.0, -yb]])
        Ga = np.hstack([-_skew(Xa), np.eye(3)])
        Gb = np.hstack([-_skew(Xb), np.eye(3)])
        want = Ga.T @ (Pa.T @ M @ Pb) @ Gb

        U = M @ Pb                                                          # rows u_0, u_1
        V = np.array([np.concatenate([np.cross(Xb, U[r]), U[r]]) for r in range(2)])
        a0, a1, a2 = Xa
        alpha = np.array([-a1 * xa, a2 + a0 * xa, -a1, 1.0, 0.0, -xa])
        beta = np.array([-a1 * ya - a2, a0 * ya, a0, 0.0, 1.0, -ya])
        got = np.outer(alpha, V[0]) + np.outer(beta, V[1])
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
