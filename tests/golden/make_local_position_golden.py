"""tests/golden/make_local_position_golden.py -- fixture for Map.getLocalPosition (Track.py:191-290) and Map.getAngle (Track.py:312-349).

Imports and EXECUTES the reference's own `Map` (read-only import from /root/reference, no bytecode written), with Track.pdb.set_trace replaced by a no-op (the
reference stops in the debugger when epsi > 1 and when a point is off the track) and its "POINT OUT OF THE TRACK" message captured, and stores inputs and outputs in
tests/golden/local_position/track_local.npz (a directory of its own: tests/golden/MANIFEST.json lists the files directly under tests/golden/,
and tests/test_track_inverse_host.py holds this fixture's content hash and this script's blob hash itself).  Run in the build container only (the GPU box has no /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_local_position_golden.py

Populations (max_ey = halfWidth + slack = 0.85 is recorded in the file):
  (a) interior points: s uniform on [0, TL) at least 1e-3 from every segment boundary, ey uniform in +-0.8, epsi uniform in +-0.9; (x, y) from Map.getGlobalPosition,
      psi from Map.getAngle, outputs from Map.getLocalPosition.  Asserted here: every point completes, on its own segment, within 1e-12 of the inputs.
  (b) the exact end point of every track row as stored in the table (= the start point of the next row): the equality branches; only those on which the reference
      returns without an exception are kept.  b_row: the first row in table order that has the point as its start or its end.
  (c) about 50 points 2 m to 5 m from the centre line: CompletedFlag == 0 and 10000 three times (asserted here).
  (d) the (a) points with psi shifted by -4 pi, -2 pi, +2 pi, +4 pi (the plant's psi is not wrapped).  s, ey and the flag are asserted here to be bit for bit those of
      (a) -- x and y are the same doubles --, so only epsi is stored: d_epsi[k] belongs to d_shift[k].
  (e) about 600 (s, epsi) samples of Map.getAngle over three laps of s, away from s = k TL (there the wrapped s is TL exactly: no segment, the reference raises).
"""
import contextlib
import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference/src/fnc/simulator"
sys.path.insert(0, REF)
import Track  # noqa: E402
from Track import Map  # noqa: E402

Track.pdb.set_trace = lambda *a, **k: None

m = Map(0.4)
pt = m.PointAndTangent.copy(); TL = float(m.TrackLength)
MAX_EY = float(m.halfWidth + m.slack)
rng = np.random.default_rng(20261018)
sink = io.StringIO()


def local(x, y, psi):
    with contextlib.redirect_stdout(sink):
        s, ey, epsi, ok = m.getLocalPosition(float(x), float(y), float(psi))
    return [float(s), float(ey), float(epsi), float(ok)]


# (a)
s = rng.uniform(0.0, TL, 4000)
edges = np.concatenate([pt[:, 3], [TL]])
s = s[np.abs(s[:, None] - edges[None]).min(axis=1) >= 1e-3]
n = s.size
ey = rng.uniform(-0.8, 0.8, n); epsi = rng.uniform(-0.9, 0.9, n)
xy = np.array([m.getGlobalPosition(float(a), float(b)) for a, b in zip(s, ey)])
psi = np.array([float(m.getAngle(float(a), float(b))) for a, b in zip(s, epsi)])
a_out = np.array([local(xy[i, 0], xy[i, 1], psi[i]) for i in range(n)])
a_row = np.array([int(np.nonzero((v >= pt[:, 3]) & (v < pt[:, 3] + pt[:, 4]))[0][0]) for v in s])
assert np.all(a_out[:, 3] == 1), "an interior point did not complete"
back_row = np.array([int(np.nonzero((v >= pt[:, 3]) & (v < pt[:, 3] + pt[:, 4]))[0][0]) for v in a_out[:, 0]])
assert np.array_equal(back_row, a_row), "an interior point completed on a neighbouring segment"
rt = max(np.abs(a_out[:, 0] - s).max(), np.abs(a_out[:, 1] - ey).max(), np.abs(a_out[:, 2] - epsi).max())
assert rt < 1e-12, rt
print("(a) %d of %d points complete on their own segment, round trip %.2e" % (int(a_out[:, 3].sum()), n, rt))

# (b)
bx, by, bpsi, b_out, b_row = [], [], [], [], []
R = pt.shape[0]
for k in range(R):
    for h in (0.0, 0.3):
        try:
            o = local(pt[k, 0], pt[k, 1], pt[k, 2] + h)
        except Exception as e:                       # (recorded only where the reference returns)
            print("(b) row %d: the reference raises %s" % (k, type(e).__name__)); continue
        bx.append(pt[k, 0]); by.append(pt[k, 1]); bpsi.append(pt[k, 2] + h); b_out.append(o)
        first = min(i for i in range(R) if (pt[i, 0], pt[i, 1]) == (pt[k, 0], pt[k, 1]) or (pt[i - 1, 0], pt[i - 1, 1]) == (pt[k, 0], pt[k, 1]))
        b_row.append(first)
b_out = np.array(b_out)
assert np.all(b_out[:, 3] == 1) and np.all(b_out[:, 1] == 0)

# (c)
dense = np.array([m.getGlobalPosition(float(v), 0.0) for v in np.linspace(0.0, TL, 4000, endpoint=False)])
lo, hi = dense.min(axis=0) - 5.0, dense.max(axis=0) + 5.0
cand = rng.uniform(lo, hi, (4000, 2))
dist = np.sqrt(((cand[:, None, :] - dense[None]) ** 2).sum(-1)).min(axis=1)
cxy = cand[(dist >= 2.0) & (dist <= 5.0)][:50]
cpsi = rng.uniform(-np.pi, np.pi, cxy.shape[0])
c_out = np.array([local(cxy[i, 0], cxy[i, 1], cpsi[i]) for i in range(cxy.shape[0])])
assert np.all(c_out[:, 3] == 0) and np.all(c_out[:, :3] == 10000.0)
assert sink.getvalue().count("POINT OUT OF THE TRACK") == cxy.shape[0]

# (d)
d_shift = np.array([-4 * np.pi, -2 * np.pi, 2 * np.pi, 4 * np.pi])
d_epsi = np.zeros((4, n))
for k, sh in enumerate(d_shift):
    o = np.array([local(xy[i, 0], xy[i, 1], psi[i] + sh) for i in range(n)])
    assert np.array_equal(o[:, [0, 1, 3]], a_out[:, [0, 1, 3]])
    d_epsi[k] = o[:, 2]
print("(d) worst |epsi(shifted) - epsi| %.2e" % np.abs(d_epsi - a_out[None, :, 2]).max())

# (e)
es = np.concatenate([np.linspace(0.0, 3.0 * TL, 400, endpoint=False), rng.uniform(0.0, 3.0 * TL, 200)])
es = es[(es == 0) | (np.abs(es / TL - np.round(es / TL)) > 1e-9)]
eepsi = rng.uniform(-0.9, 0.9, es.size)
epsi_out = np.array([float(m.getAngle(float(a), float(b))) for a, b in zip(es, eepsi)])

out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "local_position", "track_local.npz")
os.makedirs(os.path.dirname(out), exist_ok=True)
np.savez_compressed(out, track=pt, trackLength=TL, max_ey=MAX_EY,
                    a_s=s, a_ey=ey, a_epsi=epsi, a_x=xy[:, 0], a_y=xy[:, 1], a_psi=psi, a_out=a_out, a_row=a_row,
                    b_x=np.array(bx), b_y=np.array(by), b_psi=np.array(bpsi), b_out=b_out, b_row=np.array(b_row),
                    c_x=cxy[:, 0], c_y=cxy[:, 1], c_psi=cpsi, c_out=c_out,
                    d_shift=d_shift, d_epsi=d_epsi,
                    e_s=es, e_epsi=eepsi, e_psi=epsi_out)
print("wrote", out, "a", n, "b", len(bx), "c", cxy.shape[0], "d", d_epsi.size, "e", es.size, "bytes", os.path.getsize(out))
