#!/usr/bin/env python3
"""The column loop's outputs on seeded cases, one SHA-256 line each (GPU box): run it in two checkouts and diff the lines to
hold a change of the loop kernels to "bit for bit".  Covers the general window kernel (SLK_NO_WINDOW2) at several widths,
blockings and codebooks with ragged row tiles and the carried row error, k_gptq_window2 with 16 and 32 rows, grouped and
asymmetric layers with their tables in LDS and in memory (G > GSLOTS), and leaves wider than the window's 512 columns."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from sleekit_amd import _lib, engine, codebook

def sha(t):
    return "-" if t is None else hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]

def make(R, n, seed, perm=True):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((R, n)) * 0.6).astype(np.float32)
    U = np.triu(rng.standard_normal((n, n)) * (0.3 / np.sqrt(n))) + np.diag(1.0 + rng.random(n))
    order = rng.permutation(n).astype(np.int64) if perm else None
    d = lambda x: None if x is None else torch.from_numpy(x).cuda().contiguous()
    return rng, d(W), d(U), d(order)

def run(tag, R, n, mb, nb, cb, seed, opts=(), g=0, asym=False, perm=True, H=False):
    rng, W, U, order = make(R, n, seed, perm)
    kw = {}
    if g:
        kw["gscale"] = torch.from_numpy((0.5 + rng.random((R, n // g))).astype(np.float32)).cuda()
        kw["group_size"] = g
        if asym:
            kw["goffset"] = torch.from_numpy((rng.standard_normal((R, n // g)) * 0.2).astype(np.float32)).cuda()
    if H:
        A = rng.standard_normal((n, n)).astype(np.float32)
        kw["Hs"] = [torch.from_numpy(((A + A.T) / 2).astype(np.float32)).cuda().contiguous()]
        kw["damp"] = 0.01
    for k, v in opts:
        _lib.set_option(k, v)
    Q, idx, E, rerr = engine.gptq_loop(W, cb._abi(), order, U, mb, nb, want_E=True, **kw)
    torch.cuda.synchronize()
    for k, v in opts:
        _lib.set_option(k, 0)
    print(f"{tag:28s} Q {sha(Q)} idx {sha(idx)} E {sha(E)} err {sha(rerr)}", flush=True)

u8, nf4 = codebook.UniformCodebook(8, -1, 1), codebook.Codebook.nf4()
NO2 = (("SLK_NO_WINDOW2", 1),)
run("general 1376", 100, 1376, 32, 8, u8, 1, NO2)
run("general 4096", 109, 4096, 32, 8, u8, 2, NO2)
run("general 173 mb7", 40, 173, 7, 2, u8, 3, NO2)
run("general 96 mb3 noperm", 17, 96, 3, 2, u8, 4, NO2, perm=False)
run("general 1024 nf4", 33, 1024, 32, 8, nf4, 5, NO2)
run("general 768 mb64", 64, 768, 64, 4, u8, 6, NO2)
run("general 1022 mb1 nb2", 20, 1022, 1, 2, u8, 7, NO2)
run("general 3072 err", 64, 3072, 32, 8, u8, 8, NO2, H=True)
run("window2 rows16 4096", 109, 4096, 32, 8, u8, 9, (("SLK_WINDOW_ROWS", 16),))
run("window2 rows32 4096", 109, 4096, 32, 8, u8, 9, (("SLK_WINDOW_ROWS", 32),))
run("window2 rows32 1376 nf4", 70, 1376, 32, 8, nf4, 10, (("SLK_WINDOW_ROWS", 32),))
run("window2 3072 err", 2048, 3072, 32, 8, u8, 11, H=True)
run("grouped 1024 g128", 70, 1024, 32, 8, u8, 12, g=128)
run("grouped 1376 g32 nf4", 40, 1376, 32, 8, nf4, 13, g=32)
run("asym 1024 g128", 70, 1024, 32, 8, u8, 14, g=128, asym=True)
run("asym 1024 g2 (memory)", 40, 1024, 32, 8, u8, 15, g=2, asym=True)
run("grouped 4096 g128", 128, 4096, 32, 8, u8, 16, g=128)
run("asym 4096 g4096", 128, 4096, 32, 8, u8, 17, g=4096, asym=True)
run("wide 768", 40, 768, 1000, 8, u8, 18)
run("wide 513 nf4", 17, 513, 513, 8, nf4, 19)
run("wide 768 g128", 40, 768, 1000, 8, u8, 20, g=128)
run("wide 600 g100 asym", 40, 600, 1000, 8, u8, 21, g=100, asym=True)
run("leaf 512 one leaf", 40, 512, 1000, 8, u8, 22)
