"""The pick rule of the PGX playouts (envpool_amd/csrc/pgx_playout.hip.h, DESIGN.md "PGX playouts") restated in
Python integers and numpy, independently of the header: what the playout tests compute their expected values with."""
import numpy as np

M64 = (1 << 64) - 1


def sm(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def stream(seed, env_id, r):
    """The stream of repeat r of the env with the GLOBAL id env_id."""
    return sm((seed & M64) ^ sm(((int(env_id) & 0xFFFFFFFF) << 32) | (int(r) & 0xFFFFFFFF)))


def pick(mask, h, t):
    """The action of ply t of stream h on a position with the boolean legal mask `mask`."""
    legal = np.flatnonzero(mask)
    u = sm((h + t) & M64)
    return int(legal[((u >> 32) * len(legal)) >> 32])
