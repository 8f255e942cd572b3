"""The premise of the beam cull (DESIGN.md 4.2 "Beam cull"; profiles/r28_beam_cull.txt section 1), on the CPU: how much of the primary launch's work is spent on
pixels that a per-tile beam cull would finish in front of it?  For the bench view (bench.py's configs[1]: the close-up camera, 1920x1080, batches of 8) it sets
the host definition of the cull (rt.beam_cull, K sub-frames' jitters) against the oracle's primary fetches and hit pixels per 16x16 tile (orc.render with region=,
GI and AO off, one thread, one frame index), and reports

  dead tiles, the pixels in them,
  F_dead / F_all: the share of all primary fetches that pixels of dead tiles make,
  F_miss / F_all: the same share for all missing pixels -- the ceiling a finer beam could reach,

and, when F_miss - F_dead exceeds F_dead / 2, the same for 8x8 sub-beams (rt.beam_walk over the quadrants' own intervals).

    python tools/beam_cull_premise.py [--size 1920x1080] [--batch 8] [--frame 0] [--subdiv 6] [--camera closeup]
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import opengl_raytracing_amd as rt, oracle as orc, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--frame", type=int, default=0)
ap.add_argument("--subdiv", type=int, default=6)
ap.add_argument("--camera", default="closeup")
a = ap.parse_args()
W, H = map(int, a.size.split("x"))
K = a.batch

nodes, tris = scenes.bunny_bvh(a.subdiv)
cam = scenes.camera(a.camera, aspect=W / H)
p = rt.default_render_params()
p.sppPerFrame = 1
us = [rt.frame_uniforms(p, cam, W, H, a.frame + k, True, nodes.shape[0], tris.shape[0], env_loaded=False) for k in range(K)]   # (no primary fetch looks at the sky)
jit = np.array([[u.jitter[0], u.jitter[1]] for u in us], np.float32)
packed = rt.pack_scene(nodes, tris)
t0 = time.time()
dead, stats, rd = rt.beam_cull(us[0], nodes, tris, jitters=jit, rays=True, packed=packed)
t_cull = time.time() - t0
info, _ = rt.frame_geom(W, H)
tx_n, ty_n = info.tilesX, info.tilesY
assert dead.size == tx_n * ty_n

# the oracle per tile: primary fetches and hit pixels of the frame `--frame`, no GI, no AO (neither changes a primary fetch)
u = us[0]
u.enableGI = 0
u.enableAO = 0
fetch = np.zeros(dead.size, np.int64)
hits = np.zeros(dead.size, np.int64)
pix = np.zeros(dead.size, np.int64)
t0 = time.time()
for t in range(dead.size):
    ty, tx = divmod(t, tx_n)
    x0, y0, x1, y1 = tx * 16, ty * 16, min(tx * 16 + 16, W), min(ty * 16 + 16, H)
    _, cnt = orc.render(u, nodes, tris, None, None, region=(x0, y0, x1, y1), nthreads=1)
    fetch[t], hits[t], pix[t] = cnt.fetchPrimary, cnt.hitPixels, (x1 - x0) * (y1 - y0)
t_orc = time.time() - t0

F_all = int(fetch.sum())
d = dead != 0
F_dead = int(fetch[d].sum())
# fetches of missing pixels: exact for tiles without a hit; a mixed tile's fetches cannot be split per pixel from the tile counters, so the ceiling is bracketed
nohit = hits == 0
F_miss_lo = int(fetch[nohit].sum())
mixed = (~nohit) & (hits < pix)
print(f"view: {a.camera} camera, {W}x{H}, bunny subdiv {a.subdiv} ({tris.shape[0]} triangles, {nodes.shape[0]} nodes), frame {a.frame}, K = {K} sub-frames' jitters")
print(f"tiles {dead.size}: dead {int(d.sum())} ({d.mean():.4f}), kept by overflow {stats.overflowTiles}, levels walked {stats.levels} ({stats.levels / dead.size:.2f} per tile); host cull {t_cull:.2f} s, oracle {t_orc:.1f} s")
print(f"pixels {int(pix.sum())}: in dead tiles {int(pix[d].sum())} ({pix[d].sum() / pix.sum():.4f}); hit pixels {int(hits.sum())} ({hits.sum() / pix.sum():.4f}); hit pixels in dead tiles {int(hits[d].sum())} (must be 0)")
print(f"tiles without a hit {int(nohit.sum())}, mixed tiles {int(mixed.sum())} ({int((pix - hits)[mixed].sum())} missing pixels in them), all-hit tiles {int((hits == pix).sum())}")
print(f"primary fetches F_all {F_all} ({F_all / pix.sum():.2f} per pixel); per pixel of dead tiles {F_dead / max(pix[d].sum(), 1):.2f}, of no-hit tiles {F_miss_lo / max(pix[nohit].sum(), 1):.2f}, of tiles with a hit {fetch[~nohit].sum() / max(pix[~nohit].sum(), 1):.2f}")
print(f"F_dead / F_all = {F_dead / F_all:.4f}")
# missing pixels of mixed tiles: charged the tile's mean fetches per pixel (upper estimate: a miss near the silhouette walks about as deep as a hit)
F_miss_hi = F_miss_lo + int((fetch[mixed] * ((pix - hits)[mixed] / pix[mixed])).sum())
print(f"F_miss / F_all = {F_miss_lo / F_all:.4f} (tiles without a hit alone) .. {F_miss_hi / F_all:.4f} (+ the missing pixels of mixed tiles at their tile's mean)")
print(f"premise (F_dead / F_all >= 0.20): {'holds' if F_dead / F_all >= 0.20 else 'FAILS'}")

if F_miss_hi - F_dead > F_dead / 2:
    # 8x8 sub-beams: each quadrant of a kept tile with its own interval over the K sub-frames; the fetches of a quadrant come from the oracle per quadrant
    ro = np.array(list(u.camPos), np.float32)
    quads, Ls, Hs = [], [], []
    for t in np.nonzero(~d)[0]:
        ty, tx = divmod(int(t), tx_n)
        for q in range(4):
            x0, y0 = tx * 16 + (q & 1) * 8, ty * 16 + (q >> 1) * 8
            x1, y1 = min(x0 + 8, W), min(y0 + 8, H)
            if x0 >= x1 or y0 >= y1:
                continue
            r = rd[:, y0:y1, x0:x1, :].reshape(-1, 3)
            quads.append((x0, y0, x1, y1)); Ls.append(r.min(0)); Hs.append(r.max(0))
    verdict, _ = rt.beam_walk(ro, np.array(Ls), np.array(Hs), packed=packed)
    qd = np.nonzero(verdict == 0)[0]
    F_q, P_q = 0, 0
    for i in qd:
        _, cnt = orc.render(u, nodes, tris, None, None, region=quads[i], nthreads=1)
        assert cnt.hitPixels == 0
        F_q += cnt.fetchPrimary
        P_q += (quads[i][2] - quads[i][0]) * (quads[i][3] - quads[i][1])
    print(f"8x8 sub-beams over the {int((~d).sum())} kept tiles: {len(quads)} quadrants, dead {qd.size}, pixels in them {P_q}, kept by overflow {int((verdict == 2).sum())}")
    print(f"F_dead8 / F_all = {F_q / F_all:.4f} on top of the tiles' {F_dead / F_all:.4f} (worth building only if >= {F_dead / F_all:.4f} again)")
else:
    print("8x8 sub-beams: not evaluated (F_miss - F_dead <= F_dead / 2)")
