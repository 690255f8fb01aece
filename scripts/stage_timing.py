"""Per-stage cycle totals of resolve_boxes_kernel (build with `make -C art_planner_amd/csrc timing`,
which writes libartp_timing.so; the shipped libartp.so carries no instrumentation).
usage: ARTP_LIB=art_planner_amd/csrc/libartp_timing.so python scripts/stage_timing.py"""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from art_planner_amd import _capi
from art_planner_amd.context import Context
from synthetic import make_map

gm = make_map(400, 0.04, seed=1234)
ctx = Context(0, "yaml")
ctx.upload_map(gm)
L = _capi.load()
n = 1 << 22
se3 = torch.empty((n, 7), dtype=torch.float64, device="cuda:0")
va = torch.empty(n, dtype=torch.uint8, device="cuda:0")
ctx.use_torch_stream()
ctx.sample_and_validate_dev(1234, 0, n, se3, va)
torch.cuda.synchronize()
out = (C.c_ulonglong * 20)()
L.artp_debug_stage_cycles(out, 1)
ctx.sample_and_validate_dev(1234, n, n, se3, va)
torch.cuda.synchronize()
L.artp_debug_stage_cycles(out, 0)
a = np.array(list(out), dtype=np.float64).reshape(2, 10)
names = ["record", "scan", "vertex(f)", "compact", "corners"]
cnt = ctx.pipeline_counters()
print("counters", cnt)
tc = (C.c_ulonglong * 20)()
L.artp_debug_stage_cycles(tc, 7)  # 7: the torso stream pass's box counters of the second batch (read + reset)
t_taken, t_skip, t_fwd, t_vhit, t_corner, t_r1, t_r2 = (int(tc[k]) for k in range(7))
t_stream = t_taken - t_fwd
print("torso stream pass: boxes taken", t_taken, "skipped (state already failed)", t_skip, "forwarded without a stream", t_fwd,
      "streamed", t_stream, "stream hits", t_vhit, "boxes that ran the corner stage", t_corner, "corner result 0", t_corner - t_r1 - t_r2,
      "1 (contact)", t_r1, "2 (may have partners)", t_r2)
# ticks summed over the wavefronts: [0] record, [2] stream, [4] corner stage, [6] chunk fetch (flush, cursor, the chunk's
# headers), [8] lifetime (the near-empty G = 64 fallback launches add theirs to the same row)
print("  ticks: record %.0f stream %.0f corner %.0f chunk fetch %.0f lifetime %.0f" % (a[0, 0], a[0, 2], a[0, 4], a[0, 6], a[0, 8]))
print("  share of the lifetime: record %.3f stream %.3f corner %.3f chunk fetch %.3f" % tuple(a[0, k] / max(a[0, 8], 1) for k in (0, 2, 4, 6)))
print("  ticks per box: record %.0f, stream %.0f per streamed box, corner stage %.0f per box that ran it; chunk fetch %.0f per box queued"
      % (a[0, 0] / max(t_taken, 1), a[0, 2] / max(t_stream, 1), a[0, 4] / max(t_corner, 1), a[0, 6] / max(t_taken + t_skip, 1)))
ff = (C.c_ulonglong * 20)()
L.artp_debug_stage_cycles(ff, 3)  # reset >= 3: the feet_stream counters
print("feet_stream: stream ticks", ff[0], "corner ticks", ff[1], "boxes that ran the second stage", ff[2], "boxes that ran the corner stage", ff[3],
      "corner result 1 (contact)", ff[4], "2 (may have partners)", ff[5], "streams that found a vertex", ff[6])
# the pre-pass (two lanes per box, the lowest corner) runs first; ticks are per wavefront here, per 16-lane group above
live, settled, border, pre_ticks, rounds, face = (int(ff[k]) for k in range(7, 13))
print("  pre-pass: boxes live %d, settled %d (X = %.3f of the live), refused at a cell border %d, ticks %d (%.0f per live box), "
      "corner rounds %d (%.2f per chunk of 32 live boxes); the four bottom-face corners would settle %d (X = %.3f)"
      % (live, settled, settled / max(live, 1), border, pre_ticks, pre_ticks / max(live, 1), rounds, rounds * 32 / max(live, 1),
         face, face / max(live, 1)))
# the boxes that ran the second stage are the streamed ones
n_stream, n_corner = ff[2], ff[3]
print("  per box: stream (S) %.0f ticks, corner stage (C) %.0f ticks, C / S %.2f; of the boxes that ran the corner stage: streamed "
      "%.3f, contact %.3f, partners %.3f; vertex %.3f of the streamed"
      % (ff[0] / max(n_stream, 1), ff[1] / max(n_corner, 1), (ff[1] / max(n_corner, 1)) / max(ff[0] / max(n_stream, 1), 1e-9),
         n_stream / max(ff[3], 1), ff[4] / max(ff[3], 1), ff[5] / max(ff[3], 1), ff[6] / max(n_stream, 1)))
ctx.sample_and_validate_dev(1234, n, n, se3, va)
torch.cuda.synchronize()
cc = (C.c_ulonglong * 20)()
L.artp_debug_stage_cycles(cc, 2)  # reset >= 2: read the classify phase counters instead (and reset all)
c = np.array(list(cc)[:16], dtype=np.float64).reshape(2, 8)
ph = ["PoseRec load+barrier", "head", "2 barriers", "stage+barrier", "tail: record + exact statistics", "tail: exits, probe, label", "queue+copy"]
for g, nm in ((0, "classify list waves"), (1, "classify early-exit waves")):
    tot = c[g, :7].sum()
    print(nm, int(c[g, 7]), "waves, ticks/wave", round(tot / max(c[g, 7], 1)),
          {k: round(float(c[g, j] / max(c[g, 7], 1))) for j, k in enumerate(ph)})
for g, nm in ((0, "torso G=64"), (1, "feet G=16")):
    tot = a[g, :5].sum()
    print(nm, "stage ticks/lifetime", round(tot / a[g, 8], 3), "groups", int(a[g, 9]), "ticks per group", a[g, 8] / a[g, 9],
          {names[k]: round(float(a[g, k] / tot), 3) for k in range(5)},
          "corners split", {n2: round(float(a[g, k] / tot), 3) for k, n2 in ((5, "candidates"), (6, "partners"), (7, "contacts"))})
