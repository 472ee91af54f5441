"""Dense numpy model of the immersed-boundary operators on a uniform node lattice (nodes lower + i h, x fastest): the discrete
deltas phi, the weights W [markers, nodes], H = W, S = (W c)^T, A = H S (dense and in its separable closed form), and the circle."""
import numpy as np


def phi(r, kernel="four"):
    a = np.abs(np.asarray(r, dtype=float))
    with np.errstate(invalid="ignore"):
        if kernel == "four":       # Peskin, support |r| < 2
            inner = (3 - 2 * a + np.sqrt(1 + 4 * a - 4 * a * a)) / 8
            outer = (5 - 2 * a - np.sqrt(-7 + 12 * a - 4 * a * a)) / 8
            return np.where(a < 1, inner, np.where(a < 2, outer, 0.0))
        inner = (1 + np.sqrt(1 - 3 * a * a)) / 3       # Roma et al., support |r| < 3/2
        outer = (5 - 3 * a - np.sqrt(1 - 3 * (1 - a) ** 2)) / 6
        return np.where(a <= 0.5, inner, np.where(a < 1.5, outer, 0.0))


def weights_1d(X, lower, h, n, kernel="four"):
    """per axis d: [markers, n_d] = phi(((lower_d + i h_d) - X_kd) / h_d)"""
    return [phi(((lower[d] + np.arange(n[d]) * h[d])[None, :] - X[:, d:d + 1]) / h[d], kernel) for d in range(X.shape[1])]


def weights(X, lower, h, n, kernel="four"):
    """W [markers, prod n], node = ix + n_x (iy + n_y iz)"""
    W = np.ones((X.shape[0], 1))
    for w1 in weights_1d(X, lower, h, n, kernel):
        W = (w1[:, :, None] * W[:, None, :]).reshape(X.shape[0], -1)
    return W


def operators(X, dl, lower, h, n, kernel="four"):
    """H [M, N], S [N, M], A = H S [M, M]"""
    W = weights(X, lower, h, n, kernel)
    S = (W * (np.asarray(dl) / np.prod(h))[:, None]).T
    return W, S, W @ S


def matrix_closed(X, dl, lower, h, n, kernel="four"):
    """A_kl = c_l prod_d sum_i phi(r_ik) phi(r_il)"""
    A = np.tile((np.asarray(dl) / np.prod(h))[None, :], (X.shape[0], 1))
    for w1 in weights_1d(X, lower, h, n, kernel):
        A = A * (w1 @ w1.T)
    return A


def circle(center, radius, h, spacing=1.5):
    """markers [M, 2] and dl: M = round(2 pi r / (spacing h)), dl = 2 r sin(pi / M)"""
    M = int(round(2 * np.pi * radius / (spacing * h)))
    ang = 2 * np.pi * np.arange(M) / M
    X = np.asarray(center, dtype=float)[None, :] + radius * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return X, np.full(M, 2 * radius * np.sin(np.pi / M))
