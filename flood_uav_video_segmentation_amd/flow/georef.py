"""The ground model of a mosaic: what takes a pixel of the written mosaic or orthophoto to eastings and northings in
metres of a projected CRS.  Host only, float64 throughout: a model is fitted to control points (similarity, affine or projective) or
taken from telemetry, and handed to the device as two sets of nine float64 -- the forward model from ANCHOR pixel coordinates to
MILLIMETRES about a ground origin, and its inverse -- so that the device sees small numbers.  No projection library and no lon/lat:
the CRS is a name that is written through to the files.

A planar model over the mosaic's affine pose chain: the chain's drift and the parallax of anything above the ground are in the result.
No DEM, no lens model.  Not validated on real video or against surveyed points."""
import math

import numpy as np

KINDS = {"similarity": 2, "affine": 3, "projective": 4}  # the fewest control points of each kind


class GroundModel:
    """forward: nine float64, anchor pixel coordinates (i, j) -> millimetres east and north of `origin_en` as (a0 i + a1 j + a2) / (c0 i +
    c1 j + c2) and likewise with b; inverse: numpy.linalg.inv of it, computed once; origin_en: (E, N) float64 metres; kind; residuals:
    float64 [points, 2] metres (fitted minus given) and rms; crs: a name or None."""

    def __init__(self, forward, origin_en, kind="affine", residuals=None, crs=None):
        self.forward = np.asarray(forward, np.float64).reshape(9).copy()
        if not np.isfinite(self.forward).all():
            raise ValueError(f"GroundModel: the model is not finite: {self.forward.tolist()}")
        matrix = self.forward.reshape(3, 3)
        if abs(np.linalg.det(matrix)) == 0.0 or not np.isfinite(np.linalg.cond(matrix)):
            raise ValueError(f"GroundModel: the model cannot be inverted: {self.forward.tolist()}")
        self.inverse = np.linalg.inv(matrix).reshape(9)
        if not np.isfinite(self.inverse).all():
            raise ValueError(f"GroundModel: the model's inverse is not finite: {self.forward.tolist()}")
        self.origin_en = (float(origin_en[0]), float(origin_en[1]))
        if not all(math.isfinite(v) for v in self.origin_en):
            raise ValueError(f"GroundModel: the ground origin is not finite: {self.origin_en}")
        self.kind, self.crs = str(kind), None if crs is None else str(crs)
        self.residuals = np.zeros((0, 2), np.float64) if residuals is None else np.asarray(residuals, np.float64).reshape(-1, 2)
        self.rms = float(np.sqrt((self.residuals ** 2).sum(axis=1).mean())) if len(self.residuals) else 0.0

    # ---- making one
    @classmethod
    def fit(cls, canvas_xy, ground_en, kind="affine", origin=(0, 0), crs=None):
        """canvas_xy: [points, 2] continuous canvas coordinates (x to the right, y down; pixel i covers [i, i+1)) of the written mosaic or
        orthophoto; ground_en: [points, 2] eastings and northings in metres; origin = (oy, ox), the canvas' origin (the builder's `at`, a
        part's "origin").  similarity: 2 or more points, four degrees of freedom, the y-down / north-up reflection built in; affine: 3 or
        more, least squares; projective: 4 or more, the normalised DLT.  ValueError names too few points, collinear points or a result
        that is not finite."""
        if kind not in KINDS:
            raise ValueError(f"GroundModel.fit: kind must be one of {sorted(KINDS)}, got {kind!r}")
        xy, en = np.asarray(canvas_xy, np.float64), np.asarray(ground_en, np.float64)
        if xy.ndim != 2 or xy.shape[1] != 2 or en.shape != xy.shape:
            raise ValueError(f"GroundModel.fit: canvas_xy and ground_en must both be [points, 2], got {xy.shape} and {en.shape}")
        if not np.isfinite(xy).all() or not np.isfinite(en).all():
            raise ValueError("GroundModel.fit: a control point is not finite")
        if len(xy) < KINDS[kind]:
            raise ValueError(f"GroundModel.fit: a {kind} model needs {KINDS[kind]} or more control points, got {len(xy)}")
        oy, ox = (int(v) for v in origin)
        ij = xy - np.array([ox, oy], np.float64)                           # anchor coordinates
        ground_origin = np.round(en.mean(axis=0))                           # whole metres
        centre, spread = ij.mean(axis=0), float(np.abs(ij - ij.mean(axis=0)).max())
        scale_en = float(np.abs(en - ground_origin).max())
        if spread == 0.0 or scale_en == 0.0 or float(np.abs(en - en[0]).max()) == 0.0:
            raise ValueError("GroundModel.fit: the control points coincide")
        p, q = (ij - centre) / spread, (en - ground_origin) / scale_en    # both of size one: the systems below are well scaled
        sv = np.linalg.svd(p - p.mean(axis=0), compute_uv=False)
        if kind != "similarity" and sv[1] <= 1e-9 * sv[0]:
            raise ValueError("GroundModel.fit: the control points are collinear")
        ones, zeros = np.ones(len(p)), np.zeros(len(p))
        if kind == "similarity":      # E = a x + b y + tx, N = b x - a y + ty: a rotation and scale with y down and north up
            rows = np.concatenate([np.stack([p[:, 0], p[:, 1], ones, zeros], axis=1), np.stack([-p[:, 1], p[:, 0], zeros, ones], axis=1)])
            (a, b, tx, ty), *_ = np.linalg.lstsq(rows, np.concatenate([q[:, 0], q[:, 1]]), rcond=None)
            small = np.array([[a, b, tx], [b, -a, ty], [0, 0, 1]])
        elif kind == "affine":
            design = np.stack([p[:, 0], p[:, 1], ones], axis=1)
            (a0, a1, a2), *_ = np.linalg.lstsq(design, q[:, 0], rcond=None)
            (b0, b1, b2), *_ = np.linalg.lstsq(design, q[:, 1], rcond=None)
            small = np.array([[a0, a1, a2], [b0, b1, b2], [0, 0, 1]])
        else:
            rows = []
            for (x, y), (e, n) in zip(p, q):
                rows.append([x, y, 1, 0, 0, 0, -e * x, -e * y, -e])
                rows.append([0, 0, 0, x, y, 1, -n * x, -n * y, -n])
            _, s, vt = np.linalg.svd(np.array(rows))
            if s[7] <= 1e-9 * s[0]:          # eight equations' worth of rank: the ninth direction is the model
                raise ValueError("GroundModel.fit: the control points do not determine a projective model (three or more of every four are collinear)")
            small = vt[-1].reshape(3, 3)
            if small[2, 2] == 0.0:
                raise ValueError("GroundModel.fit: the fitted projective model has no finite value at the control points' centre")
            small = small / small[2, 2]
        # anchor -> normalised pixels, the small model, normalised ground -> millimetres about the ground origin
        to_p = np.array([[1 / spread, 0, -centre[0] / spread], [0, 1 / spread, -centre[1] / spread], [0, 0, 1]])
        to_mm = np.diag([scale_en * 1000.0, scale_en * 1000.0, 1.0])
        forward = to_mm @ small @ to_p
        if not np.isfinite(forward).all() or forward[2, 2] == 0.0:
            raise ValueError(f"GroundModel.fit: the fitted model is not finite: {forward.reshape(-1).tolist()}")
        forward = forward / forward[2, 2]
        model = cls(forward, ground_origin, kind, crs=crs)
        fitted = model.to_ground(xy, origin)
        if not np.isfinite(fitted).all():
            raise ValueError("GroundModel.fit: the fitted model is not finite at a control point (its horizon crosses the points)")
        model.residuals = fitted - en
        model.rms = float(np.sqrt((model.residuals ** 2).sum(axis=1).mean()))
        return model

    @classmethod
    def from_telemetry(cls, gsd_m, heading_deg, centre_en, canvas_xy, origin=(0, 0), crs=None):
        """The nadir case without control points: a camera looking straight down, one pixel gsd_m metres a side, the image's up direction
        heading_deg degrees clockwise from north, and the canvas point canvas_xy (continuous coordinates) over centre_en.  A similarity."""
        gsd, heading = float(gsd_m), math.radians(float(heading_deg))
        if not (math.isfinite(gsd) and gsd > 0.0 and math.isfinite(heading)):
            raise ValueError(f"GroundModel.from_telemetry: gsd_m must be positive and heading_deg finite, got {gsd_m} and {heading_deg}")
        oy, ox = (int(v) for v in origin)
        ci, cj = float(canvas_xy[0]) - ox, float(canvas_xy[1]) - oy
        ground_origin = (float(round(float(centre_en[0]))), float(round(float(centre_en[1]))))
        a, b = gsd * math.cos(heading) * 1000.0, -gsd * math.sin(heading) * 1000.0   # E = a di + b dj, N = b di - a dj, in millimetres
        te, tn = (float(centre_en[0]) - ground_origin[0]) * 1000.0, (float(centre_en[1]) - ground_origin[1]) * 1000.0
        forward = [a, b, te - a * ci - b * cj, b, -a, tn - b * ci + a * cj, 0.0, 0.0, 1.0]
        return cls(forward, ground_origin, "similarity", crs=crs)

    # ---- using one on the host (float64; the device's integers are ops.ground_points')
    def to_ground(self, canvas_xy, origin=(0, 0)):
        """Continuous canvas coordinates [points, 2] -> metres (E, N) float64, unrounded."""
        xy = np.asarray(canvas_xy, np.float64).reshape(-1, 2)
        oy, ox = (int(v) for v in origin)
        m = self.forward
        i, j = xy[:, 0] - ox, xy[:, 1] - oy
        with np.errstate(all="ignore"):
            d = m[6] * i + m[7] * j + m[8]
            return np.stack([(m[0] * i + m[1] * j + m[2]) / d / 1000.0 + self.origin_en[0], (m[3] * i + m[4] * j + m[5]) / d / 1000.0 + self.origin_en[1]], axis=1)

    def mm_to_en(self, mm):
        """ops.ground_points' int64 millimetres about the ground origin -> metres (E, N) float64."""
        return np.asarray(mm, np.float64) / 1000.0 + np.array(self.origin_en, np.float64)

    def footprint_mm(self, size, origin):
        """The canvas' four corners (top-left, top-right, bottom-right, bottom-left) in millimetres about the ground origin, float64 [4, 2]."""
        ch, cw = (int(v) for v in size)
        corners = np.array([[0, 0], [cw, 0], [cw, ch], [0, ch]], np.float64)
        return (self.to_ground(corners, origin) - np.array(self.origin_en)) * 1000.0

    def mean_gsd_mm(self, size, origin):
        """The model's mean pixel size over the canvas: the square root of footprint area / pixels, rounded to whole millimetres, >= 1."""
        f = self.footprint_mm(size, origin)
        area2 = sum(f[k][0] * f[(k + 1) % 4][1] - f[(k + 1) % 4][0] * f[k][1] for k in range(4))
        gsd = math.sqrt(abs(area2) / 2.0 / (int(size[0]) * int(size[1])))
        if not math.isfinite(gsd):
            raise ValueError("GroundModel: the model has no finite footprint over this canvas")
        return max(1, int(round(gsd)))

    def raster(self, size, origin, gsd_mm=None):
        """The north-up raster that covers the canvas: (raster_size = (GH, GW), gsd_mm, top_left_mm = (E, N) of its top-left CORNER in whole
        millimetres, a multiple of gsd_mm so that rasters of one model and gsd share a grid)."""
        gsd = self.mean_gsd_mm(size, origin) if gsd_mm is None else int(gsd_mm)
        if gsd < 1:
            raise ValueError(f"GroundModel.raster: gsd_mm must be at least 1, got {gsd_mm}")
        f = self.footprint_mm(size, origin)
        if not np.isfinite(f).all():
            raise ValueError("GroundModel.raster: the model has no finite footprint over this canvas")
        slack = 1e-6   # of a raster pixel: a footprint that passes a grid line by less adds no row or column for it
        e0, e1 = math.floor(f[:, 0].min() / gsd + slack) * gsd, math.ceil(f[:, 0].max() / gsd - slack) * gsd
        n0, n1 = math.floor(f[:, 1].min() / gsd + slack) * gsd, math.ceil(f[:, 1].max() / gsd - slack) * gsd
        return (max(1, (n1 - n0) // gsd), max(1, (e1 - e0) // gsd)), gsd, (int(e0), int(n1))

    def world_file(self, gsd_mm, top_left_mm):
        """The six numbers of a raster's world file, in metres: gsd, 0, 0, -gsd, E and N of the top-left pixel's CENTRE."""
        g = gsd_mm / 1000.0
        return [g, 0.0, 0.0, -g, self.origin_en[0] + (top_left_mm[0] + gsd_mm / 2.0) / 1000.0, self.origin_en[1] + (top_left_mm[1] - gsd_mm / 2.0) / 1000.0]

    def __repr__(self):
        return f"GroundModel({self.kind}, origin_en={self.origin_en}, rms={self.rms:.4g} m, crs={self.crs!r})"


def read_gcp_csv(path, indices=False):
    """A control-point file with the columns x,y,easting,northing (a header line is optional) -> (canvas_xy, ground_en) float64 [points, 2].
    indices=True: x and y are pixel INDICES as an image viewer shows them, the pixel's centre is meant: half a pixel is added."""
    xy, en = [], []
    with open(path) as f:
        for n, line in enumerate(f):
            cells = [c.strip() for c in line.replace(";", ",").split(",")]
            if not line.strip() or line.lstrip().startswith("#"):
                continue
            try:
                x, y, e, north = (float(c) for c in cells[:4])
            except ValueError:
                if not xy and n == 0:
                    continue            # the header
                raise ValueError(f"read_gcp_csv: {path} line {n + 1} is not x,y,easting,northing: {line.strip()!r}")
            xy.append([x + 0.5, y + 0.5] if indices else [x, y])
            en.append([e, north])
    if not xy:
        raise ValueError(f"read_gcp_csv: {path} holds no control point")
    return np.array(xy, np.float64), np.array(en, np.float64)
