"""float64 specification of the code tables (csrc/code_tables.hip, include/isi_hip.h "Code tables").

dec_t's first 3x3 convolution and upsample_top_to_bottom[0] (ConvTranspose2d k4 s2 p1) read nothing but the quantised
top map, whose pixels are codebook rows E[id]; both are linear in it.  The per-code products are tabulated once,

    T3[t = kh*3 + kw][k][n]                  = sum_c W3[n][c][kh][kw] E[k][c]
    TU[ph = py*2 + px][t = ty*2 + tx][k][n]  = sum_c WT[c][n][3 - py - 2 ty][3 - px - 2 tx] E[k][c]

and the layers become sums of table rows over the taps that fall inside the map:

    conv3[b, y, x]          = bias + sum T3[t][id[b, y + kh - 1, x + kw - 1]]
    up[b, 2y + py, 2x + px] = bias + sum TU[ph][t][id[b, y - 1 + py + ty, x - 1 + px + tx]]

Everything here is float64 torch on the CPU.  The *_sum functions also return sum |terms| + |bias| per output element,
the magnitude the kernels' error bounds are stated against, and the mask of the output pixels whose window holds a code
outside [0, K) (the kernel writes NaN there; the spec's sums treat such a tap as absent)."""
import torch


def tables(w3: torch.Tensor, wT: torch.Tensor, codes: torch.Tensor):
    """w3 [Cout3, D, 3, 3], wT [D, CoutU, 4, 4], codes [K, D] -> T3 [9, K, Cout3], TU [4, 4, K, CoutU] (float64)"""
    w3, wT, e = w3.double(), wT.double(), codes.double()
    t3 = torch.stack([e @ w3[:, :, kh, kw].t() for kh in range(3) for kw in range(3)])
    tu = torch.stack([torch.stack([e @ wT[:, :, 3 - py - 2 * ty, 3 - px - 2 * tx] for ty in range(2) for tx in range(2)])
                      for py in range(2) for px in range(2)])
    return t3, tu


def _gather_shifted(rows: torch.Tensor, ids: torch.Tensor, dy: int, dx: int):
    """rows [K, C], ids [B, H, W] -> (rows[ids[b, y + dy, x + dx]] or 0 outside the map / for a bad code [B, H, W, C],
    bad [B, H, W]: the tap is inside the map and its code is outside [0, K))"""
    B, H, W = ids.shape
    K = rows.shape[0]
    out = rows.new_zeros(B, H, W, rows.shape[1])
    bad = torch.zeros(B, H, W, dtype=torch.bool)
    ys, xs = range(max(0, -dy), min(H, H - dy)), range(max(0, -dx), min(W, W - dx))
    if len(ys) == 0 or len(xs) == 0:
        return out, bad
    y0, y1, x0, x1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1
    src = ids[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    ok = (src >= 0) & (src < K)
    out[:, y0:y1, x0:x1] = rows[src.clamp(0, K - 1)] * ok.unsqueeze(-1)
    bad[:, y0:y1, x0:x1] = ~ok
    return out, bad


def conv3_sum(t3: torch.Tensor, bias: torch.Tensor, ids: torch.Tensor, relu: bool = True):
    """-> (value [B, H, W, C], magnitude |bias| + sum |terms|, bad [B, H, W])"""
    bias = bias.double()
    B, H, W = ids.shape
    val = bias.expand(B, H, W, -1).clone()
    mag = bias.abs().expand(B, H, W, -1).clone()
    bad = torch.zeros(B, H, W, dtype=torch.bool)
    for kh in range(3):
        for kw in range(3):
            term, b = _gather_shifted(t3[kh * 3 + kw].double(), ids, kh - 1, kw - 1)
            val += term
            mag += term.abs()
            bad |= b
    return (torch.relu(val) if relu else val), mag, bad


def upsample_sum(tu: torch.Tensor, bias: torch.Tensor, ids: torch.Tensor):
    """-> (value [B, 2H, 2W, C], magnitude, bad [B, 2H, 2W])"""
    bias = bias.double()
    B, H, W = ids.shape
    C = tu.shape[-1]
    val = bias.expand(B, 2 * H, 2 * W, C).clone()
    mag = bias.abs().expand(B, 2 * H, 2 * W, C).clone()
    bad = torch.zeros(B, 2 * H, 2 * W, dtype=torch.bool)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    term, b = _gather_shifted(tu[py * 2 + px][ty * 2 + tx].double(), ids, py + ty - 1, px + tx - 1)
                    val[:, py::2, px::2] += term
                    mag[:, py::2, px::2] += term.abs()
                    bad[:, py::2, px::2] |= b
    return val, mag, bad
