"""A working stand-in for `shapely.geometry.Polygon`, as far as the reference's detection code uses it (common_utils.convert_format
builds one polygon per box from four (x, y) pairs; compute_iou reads `a.intersection(b).area / a.union(b).area`).  shapely is not
installed in the build container.  Used ONLY by make_golden_detect.py, never by tests or the product.

The polygons are convex quads, so intersection is the textbook Sutherland-Hodgman clip in float64 (clip polygon made counter-clockwise
first; intersection points from the two-line determinant formula), and `union(o).area` is area + o.area - intersection area.  As for
every stand-in here, the arithmetic inside the third-party package is "parity unpinned": the fixture pins the reference's own logic
around it - candidate order, the cut at 1000, which boxes are compared, the comparisons and the bookkeeping.

install() must run BEFORE _standins.install(), which adds its inert Polygon only when `shapely` is absent from sys.modules."""
import sys
import types


def _shoelace(pts):
    s = 0.0
    for k in range(len(pts)):
        x0, y0 = pts[k - 1]
        x1, y1 = pts[k]
        s += x0 * y1 - x1 * y0
    return 0.5 * s


def _line_intersection(p1, p2, p3, p4):
    """the point where the line p1 p2 meets the line p3 p4"""
    d = (p1[0] - p2[0]) * (p3[1] - p4[1]) - (p1[1] - p2[1]) * (p3[0] - p4[0])
    a = p1[0] * p2[1] - p1[1] * p2[0]
    b = p3[0] * p4[1] - p3[1] * p4[0]
    return ((a * (p3[0] - p4[0]) - (p1[0] - p2[0]) * b) / d, (a * (p3[1] - p4[1]) - (p1[1] - p2[1]) * b) / d)


def _inside(p, a, b):
    return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) >= 0.0


class _Area(object):
    def __init__(self, area):
        self.area = area


class Polygon(object):
    def __init__(self, shell=()):
        self.pts = [(float(x), float(y)) for x, y in shell]
        self.signed = _shoelace(self.pts) if len(self.pts) >= 3 else 0.0
        xs, ys = [p[0] for p in self.pts] or [0.0], [p[1] for p in self.pts] or [0.0]
        self.bounds = (min(xs), min(ys), max(xs), max(ys))

    @property
    def area(self):
        return abs(self.signed)

    def _ccw(self):
        return self.pts if self.signed >= 0 else self.pts[::-1]

    def intersection(self, other):
        a, b = self.bounds, other.bounds
        if len(self.pts) < 3 or len(other.pts) < 3 or a[2] <= b[0] or b[2] <= a[0] or a[3] <= b[1] or b[3] <= a[1]:
            return Polygon()                         # bounding boxes apart (or touching): no area in common
        out = self._ccw()
        clip = other._ccw()
        for k in range(len(clip)):
            a, b = clip[k - 1], clip[k]
            src, out = out, []
            for i in range(len(src)):
                prev, cur = src[i - 1], src[i]
                if _inside(cur, a, b):
                    if not _inside(prev, a, b):
                        out.append(_line_intersection(prev, cur, a, b))
                    out.append(cur)
                elif _inside(prev, a, b):
                    out.append(_line_intersection(prev, cur, a, b))
            if len(out) < 3:
                return Polygon()
        return Polygon(out)

    def union(self, other):
        return _Area(self.area + other.area - self.intersection(other).area)


def install():
    sh = types.ModuleType("shapely")
    geo = types.ModuleType("shapely.geometry")
    geo.Polygon = Polygon
    sh.geometry = geo
    sh._cobevt_standin = True
    sys.modules["shapely"] = sh
    sys.modules["shapely.geometry"] = geo
