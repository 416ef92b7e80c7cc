"""Track tables from segment specs: the host-side construction of Map.__init__ (fnc/simulator/Track.py:54-133), restated from that specification -- as
tests/track_ref.py restates the inverse map -- so that a batch can be given several tracks (Context.track_set, BatchedRollouts(tracks=)).

A spec is a list of segments (length, signed radius): radius 0 is a straight, a positive radius turns left, a negative one right.  The table has one row per
segment plus the closing straight back to the origin; a row is [x, y, psi, cumulative s, segment length, signed curvature] with (x, y, psi) the pose at the END of
the segment.  Every operation is written in the order the reference evaluates it, with NumPy's scalar functions: the table of the L spec equals the reference's
bit for bit (tests/test_tracks_host.py)."""
import numpy as np

# The three specs of Track.py:15-48 as the doubles its expressions evaluate to: "L" is the live one (lengthCurve = 4.5), "goggle" and "oval" the two it carries
# in comments.  1.432394487827058 = 4.5 / pi, 2.864788975654116 = 4.5 / pi * 2 (and 60 * 0.03 * 5 / pi), 1.5278874536821951 = 80 * 0.03 * 2 / pi,
# 3.819718634205488 = 40 * 0.03 * 10 / pi, 1.7999999999999998 = 60 * 0.03.
REFERENCE_SPECS = {
    "L": [[1.0, 0.0], [4.5, 1.432394487827058], [2.25, -1.432394487827058], [4.5, 1.432394487827058], [2.864788975654116, 0.0], [2.25, 1.432394487827058]],
    "oval": [[1.0, 0.0], [4.5, -1.432394487827058], [2.0, 0.0], [4.5, -1.432394487827058], [1.0, 0.0]],
    "goggle": [[1.7999999999999998, 0.0], [2.4, -1.5278874536821951], [0.6, 0.0], [2.4, -1.5278874536821951], [1.2, 3.819718634205488],
               [1.7999999999999998, -2.864788975654116], [1.2, 3.819718634205488], [2.4, -1.5278874536821951], [0.6, 0.0], [2.4, -1.5278874536821951]],
}


def _wrap(a):
    """An angle outside [-pi, pi] moved back by one turn (Track.py:367-375)."""
    if a < -np.pi:
        return 2 * np.pi + a
    if a > np.pi:
        return a - 2 * np.pi
    return a


def table_from_spec(spec):
    """(PointAndTangent, TrackLength) of a segment spec ((n, 2): length, signed radius; n <= 15 for a context's 16 table rows)."""
    spec = np.asarray(spec, dtype=np.float64)
    if spec.ndim != 2 or spec.shape[1] != 2 or spec.shape[0] < 1:
        raise ValueError("table_from_spec: an (n, 2) array of (length, radius) expected, got shape %s" % (spec.shape,))
    n = spec.shape[0]
    tab = np.zeros((n + 1, 6))
    x0 = y0 = ang = s0 = len0 = 0.0            # pose at the start of the segment, and (cumulative s, length) of the segment before it
    for i in range(n):
        length, r = spec[i, 0], spec[i, 1]
        if i > 0:
            x0, y0, ang, s0, len0 = tab[i - 1, 0], tab[i - 1, 1], tab[i - 1, 2], tab[i - 1, 3], tab[i - 1, 4]
        if r == 0.0:                           # a straight: the heading stays
            x = x0 + length * np.cos(ang)
            y = y0 + length * np.sin(ang)
            psi, cur = ang, 0.0
        else:                                  # an arc of radius |r| about a centre a quarter turn to the left (r >= 0) or right of the heading
            d = 1 if r >= 0 else -1
            cx = x0 + np.abs(r) * np.cos(ang + d * np.pi / 2)
            cy = y0 + np.abs(r) * np.sin(ang + d * np.pi / 2)
            span = length / np.abs(r)
            psi = _wrap(ang + span * np.sign(r))
            normal = _wrap(d * np.pi / 2 + ang)
            a0 = -(np.pi - np.abs(normal)) * (1 if normal >= 0 else -1)     # direction from the centre to the start of the arc
            x = cx + np.abs(r) * np.cos(a0 + d * span)
            y = cy + np.abs(r) * np.sin(a0 + d * span)
            cur = 1 / r
        tab[i] = [x, y, psi, s0 + len0, length, cur]
    # the closing straight from the end of the last segment to the origin, heading 0
    xs, ys = tab[-2, 0], tab[-2, 1]
    tab[-1] = [0, 0, 0, tab[-2, 3] + tab[-2, 4], np.sqrt((0 - xs) ** 2 + (0 - ys) ** 2), 0]
    return tab, float(tab[-1, 3] + tab[-1, 4])
