"""The packed form of a KV slot's first positions (host-RAM tier), in plain numpy (test helper).

Written from the layout sentence, not from the device code: the packed form of the first P positions (P a multiple
of 32) of a slot is

    packed[t][layer][K|V][kv head][32 * D]   f16,  t = 0 .. P/32 - 1

where each 32 * D block is the bytes of positions [32t, 32t + 32) of that (layer, slot, kv head) region of K or of
V.  With position-major tiles those are elements [32t * D, 32(t + 1) * D) of the region, which is what tiling the
32 positions on their own with tests/kv_layout.py gives.
"""
import numpy as np

import kv_layout as L


def ceil32(n):
    return (n + 31) // 32 * 32


def tile_elems(n_layer, H, D):
    """f16 elements of one position tile of an entry."""
    return n_layer * 2 * H * 32 * D


def tile_words(n_layer, H, D):
    """... in the 16-byte words the tables count offsets in."""
    return tile_elems(n_layer, H, D) // 8


def packed_index(t, layer, kv, head, e, n_layer, H, D):
    """Element index of element e of block (t, layer, kv, head) from the start of an entry."""
    return (((t * n_layer + layer) * 2 + kv) * H + head) * 32 * D + e


def pack_entry(k, v, slot, n_pos):
    """uint16 [P/32 * tile_elems]: the packed form of slot `slot` of the logical caches k, v
    [layer][slot][kv head][position][d] (P = n_pos rounded up to 32, at most the position count)."""
    n_layer, _, H, S, D = k.shape
    P = min(ceil32(n_pos), S)
    out = np.empty((P // 32, n_layer, 2, H, 32 * D), dtype=k.dtype)
    for t in range(P // 32):
        out[t, :, 0] = L.tile_k(k[:, slot, :, 32 * t:32 * t + 32, :])
        out[t, :, 1] = L.tile_v(v[:, slot, :, 32 * t:32 * t + 32, :])
    return out.reshape(-1)
