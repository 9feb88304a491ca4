"""On-disk interchange with the reference's artefacts (host-side, no GPU work).

Writers produce byte-for-byte what the reference's writers produce, so results can be diffed against
`bunny_data/`; readers accept those files.  Reference code these mirror:

* pair files            save_pair_data            /root/reference/utils/find_matches.py:312-327
* poses/points JSON+PLY save_reconstruction/_ply  /root/reference/utils/sfm_reconstruction.py:711-767
* COLMAP text + db      SfMExporter               /root/reference/utils/export.py:9-187
* images / silhouettes  read_pnm / write_pnm      binary .ppm / .pgm, what cv2.imread returns for them

tests/test_interchange.py regenerates the five artefacts the reference ships under
bunny_data/{reconstruction,exports/colmap}/ from the shipped state and compares SHA-256 digests.
"""
from __future__ import annotations

import json
import logging
import sqlite3
from pathlib import Path

import numpy as np

COLMAP_CAMERA_LINE = "1 PINHOLE 1024 768 2393.95 2398.12 932.38 628.26"     # export.py:59 (literal)
COLMAP_CAMERA_PARAMS = (2393.95, 2398.12, 932.38, 628.26)                    # export.py:175


# ------------------------------------------------------------------------------------------- pair files
def save_pair_data(data_dir, pair_name, pts1, pts2, F, inlier_mask, matches):
    """Three files per verified pair: inlier correspondences (.npy), F + mask + all matched points (.npz),
    match indices/distances (.npz).  `matches`: objects with queryIdx / trainIdx / distance."""
    data_dir = Path(data_dir)
    corr, fund, mdir = data_dir / 'correspondences', data_dir / 'fundamental', data_dir / 'matches'
    for d in (corr, fund, mdir):
        d.mkdir(parents=True, exist_ok=True)
    inlier_mask = np.asarray(inlier_mask)
    np.save(corr / f'{pair_name}_pts1.npy', pts1[inlier_mask])
    np.save(corr / f'{pair_name}_pts2.npy', pts2[inlier_mask])
    np.savez(fund / f'{pair_name}_F.npz', F=F, mask=inlier_mask, pts1=pts1, pts2=pts2)
    if hasattr(matches, "queryIdx") and len(matches) > 0:
        # a DMatchList (sfm_amd.matcher): the arrays are there already; dtypes as np.array() of Python ints / floats gives them
        qi, ti, di = (np.asarray(matches.queryIdx, dtype=np.int64), np.asarray(matches.trainIdx, dtype=np.int64),
                      np.asarray(matches.distance, dtype=np.float64))
    else:
        qi, ti, di = (np.array([m.queryIdx for m in matches]), np.array([m.trainIdx for m in matches]),
                      np.array([m.distance for m in matches]))
    np.savez(mdir / f'{pair_name}_matches.npz', queryIdx=qi, trainIdx=ti, distance=di, inlier_mask=inlier_mask)


def load_pair_data(data_dir, pair_name):
    """Everything save_pair_data wrote for one pair (plain arrays; nothing is unpickled)."""
    data_dir = Path(data_dir)
    out = {'corr_pts1': np.load(data_dir / 'correspondences' / f'{pair_name}_pts1.npy', allow_pickle=False),
           'corr_pts2': np.load(data_dir / 'correspondences' / f'{pair_name}_pts2.npy', allow_pickle=False)}
    with np.load(data_dir / 'fundamental' / f'{pair_name}_F.npz', allow_pickle=False) as z:
        out.update(F=z['F'], mask=z['mask'], pts1=z['pts1'], pts2=z['pts2'])
    with np.load(data_dir / 'matches' / f'{pair_name}_matches.npz', allow_pickle=False) as z:
        out.update(queryIdx=z['queryIdx'], trainIdx=z['trainIdx'], distance=z['distance'],
                   inlier_mask=z['inlier_mask'])
    return out


# ---------------------------------------------------------------------------------------- reconstruction
def _plain(v):
    return v.tolist() if isinstance(v, np.ndarray) else v


def save_ply(points3D, filepath):
    pts = np.array(points3D)
    head = ["ply", "format ascii 1.0", f"element vertex {len(pts)}",
            "property float x", "property float y", "property float z", "end_header"]
    with open(filepath, 'w') as f:
        f.write("\n".join(head) + "\n")
        f.writelines(f"{p[0]} {p[1]} {p[2]}\n" for p in pts)


def save_ply_points(points, colors, path, normals=None):
    """A dense cloud as binary little-endian PLY: points [n,3] as float32 x, y, z; normals None or [n,3], written as float32
    nx, ny, nz after the coordinates; colors None, [n] gray or [n,3] uint8 in cv2's channel order (BGR), written as red,
    green, blue."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(pts)}",
            "property float x", "property float y", "property float z"]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        nrm = np.asarray(normals)
        if nrm.shape != (len(pts), 3):
            raise ValueError("normals must be [n,3], one per point")
        head += ["property float nx", "property float ny", "property float nz"]
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        col = np.asarray(colors)
        if col.dtype != np.uint8 or col.shape not in ((len(pts),), (len(pts), 3)):
            raise ValueError("colors must be uint8 [n] or [n,3], one per point")
        col = np.repeat(col[:, None], 3, axis=1) if col.ndim == 1 else col[:, ::-1]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    body = np.zeros(len(pts), dtype=np.dtype(fields))
    body["x"], body["y"], body["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if normals is not None:
        body["nx"], body["ny"], body["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colors is not None:
        body["red"], body["green"], body["blue"] = col[:, 0], col[:, 1], col[:, 2]
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii"))
        f.write(body.tobytes())


def save_ply_mesh(vertices, triangles, path, normals=None, colors=None):
    """A triangle mesh as binary little-endian PLY: the vertex element as `save_ply_points` writes it (float32 x, y, z, then
    nx, ny, nz with normals, then red, green, blue with colors), then `element face` with one `list uchar int vertex_indices`
    of three int32 per triangle.  triangles: [m,3] integers, every index below the number of vertices."""
    pts = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(triangles)
    if tri.size == 0:
        tri = np.zeros((0, 3), dtype=np.int32)
    if tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu":
        raise ValueError("triangles must be integers [m,3]")
    if len(tri) and (tri.min() < 0 or tri.max() >= len(pts)):
        raise ValueError("a triangle names a vertex that does not exist")
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(pts)}",
            "property float x", "property float y", "property float z"]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        nrm = np.asarray(normals)
        if nrm.shape != (len(pts), 3):
            raise ValueError("normals must be [n,3], one per vertex")
        head += ["property float nx", "property float ny", "property float nz"]
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        col = np.asarray(colors)
        if col.dtype != np.uint8 or col.shape not in ((len(pts),), (len(pts), 3)):
            raise ValueError("colors must be uint8 [n] or [n,3], one per vertex")
        col = np.repeat(col[:, None], 3, axis=1) if col.ndim == 1 else col[:, ::-1]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    head += [f"element face {len(tri)}", "property list uchar int vertex_indices"]
    body = np.zeros(len(pts), dtype=np.dtype(fields))
    body["x"], body["y"], body["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if normals is not None:
        body["nx"], body["ny"], body["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colors is not None:
        body["red"], body["green"], body["blue"] = col[:, 0], col[:, 1], col[:, 2]
    faces = np.zeros(len(tri), dtype=np.dtype([("n", "u1"), ("v", "<i4", 3)]))
    faces["n"], faces["v"] = 3, tri
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii"))
        f.write(body.tobytes())
        f.write(faces.tobytes())


def write_png(path, image):
    """An 8-bit gray [h,w] or RGB [h,w,3] uint8 array as a PNG file: one zlib stream of the rows, each with filter type 0,
    through the standard library alone.  The channels are written in the order they have."""
    import struct
    import zlib
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("image must be uint8 [h,w] or [h,w,3] with at least one pixel")
    h, w = img.shape[:2]
    rows = np.zeros((h, 1 + w * (3 if img.ndim == 3 else 1)), np.uint8)         # column 0: the filter type of the row, none
    rows[:, 1:] = img.reshape(h, -1)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if img.ndim == 3 else 0, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        f.write(chunk(b"IEND", b""))


def save_obj_mesh(vertices, triangles, path, normals=None, uv=None, texture=None, bgr=True):
    """A triangle mesh as Wavefront OBJ text: `v` per vertex, `vn` per vertex with normals, and with uv (float32 [m,3,2],
    per triangle corner (u, v) with v counted downwards from the top row, as `MeshTexture.uv` is) one `vt u (1 - v)` per
    corner - the format counts v upwards - and faces `f a/ta/a` (1-based; `a//a` without uv, `a/ta` without normals).  With
    texture (uint8 [h,w] or [h,w,3]) the image goes to <stem>.png and a material with `map_Kd` to <stem>.mtl, both beside
    path; bgr=True reverses the channels of a three-channel texture on the way, because the project's images are BGR."""
    path = Path(path)
    pts = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(triangles)
    if tri.size == 0:
        tri = np.zeros((0, 3), dtype=np.int32)
    if tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu":
        raise ValueError("triangles must be integers [m,3]")
    if len(tri) and (tri.min() < 0 or tri.max() >= len(pts)):
        raise ValueError("a triangle names a vertex that does not exist")
    if normals is not None and np.shape(normals) != (len(pts), 3):
        raise ValueError("normals must be [n,3], one per vertex")
    if uv is not None and np.shape(uv) != (len(tri), 3, 2):
        raise ValueError("uv must be [m,3,2], one pair per triangle corner")
    if texture is not None and uv is None:
        raise ValueError("a texture needs uv")
    lines = ["# sfm_amd mesh"]
    if texture is not None:
        img = np.asarray(texture)
        write_png(path.with_suffix(".png"), img[:, :, ::-1] if (bgr and img.ndim == 3) else img)
        with open(path.with_suffix(".mtl"), "w") as f:
            f.write(f"newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {path.with_suffix('.png').name}\n")
        lines += [f"mtllib {path.with_suffix('.mtl').name}", "usemtl atlas"]
    lines += ["v %.17g %.17g %.17g" % tuple(p) for p in pts]
    if normals is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(n) for n in np.asarray(normals, dtype=np.float64)]
    if uv is not None:
        q = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
        lines += ["vt %.9g %.9g" % (u, 1.0 - v) for u, v in q]
    for t, (a, b, c) in enumerate(tri + 1):
        if uv is not None:
            ref = (lambda i, k: f"{i}/{3 * t + k + 1}/{i}") if normals is not None else (lambda i, k: f"{i}/{3 * t + k + 1}")
        else:
            ref = (lambda i, k: f"{i}//{i}") if normals is not None else (lambda i, k: f"{i}")
        lines.append(f"f {ref(a, 0)} {ref(b, 1)} {ref(c, 2)}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def save_reconstruction(poses, points3D, point_tracks, output_dir):
    """poses.json, points3D.json (points + tracks, image ids as strings) and reconstruction.ply."""
    output_dir = Path(output_dir)
    output_dir.mkdir(exist_ok=True)
    pose_json = {str(k): {'R': np.asarray(R).tolist(), 't': np.asarray(t).ravel().tolist()}
                 for k, (R, t) in poses.items()}
    with open(output_dir / 'poses.json', 'w') as f:
        json.dump(pose_json, f, indent=2)
    body = {'points3D': [_plain(p) for p in points3D],
            'tracks': [{str(k): _plain(v) for k, v in tr.items()} for tr in point_tracks]}
    with open(output_dir / 'points3D.json', 'w') as f:
        json.dump(body, f, indent=2)
    save_ply(points3D, output_dir / 'reconstruction.ply')
    logging.info(f"Saved reconstruction to {output_dir}")


def load_reconstruction(recon_dir, int_keys=True):
    """(poses, points3D, point_tracks) from poses.json / points3D.json.  int_keys=True restores the in-memory
    form the driver uses (image ids as ints, R as arrays, t as (3,1)); False keeps the JSON strings."""
    recon_dir = Path(recon_dir)
    with open(recon_dir / 'poses.json') as f:
        raw = json.load(f)
    with open(recon_dir / 'points3D.json') as f:
        body = json.load(f)
    key = int if int_keys else str
    poses = {key(k): (np.asarray(v['R'], dtype=np.float64), np.asarray(v['t'], dtype=np.float64).reshape(3, 1))
             for k, v in raw.items()}
    tracks = [{key(k): p for k, p in tr.items()} for tr in body['tracks']]
    return poses, body['points3D'], tracks


class ReconstructionIOMixin:
    """save_reconstruction / save_ply with the reference's method signatures."""

    def save_reconstruction(self, output_dir):
        save_reconstruction(self.poses, self.points3D, self.point_tracks, output_dir)

    def save_ply(self, filepath):
        save_ply(self.points3D, filepath)


# ------------------------------------------------------------------------------------------------ COLMAP
def rotation_to_quaternion(R):
    """(qw, qx, qy, qz) by the largest-pivot branch rule of export.py:125-151."""
    R = np.asarray(R)
    d = (R[0, 0], R[1, 1], R[2, 2])
    tr = np.trace(R)
    if tr > 0:
        S = np.sqrt(tr + 1.0) * 2
        return 0.25 * S, (R[2, 1] - R[1, 2]) / S, (R[0, 2] - R[2, 0]) / S, (R[1, 0] - R[0, 1]) / S
    if d[0] > d[1] and d[0] > d[2]:
        S = np.sqrt(1.0 + d[0] - d[1] - d[2]) * 2
        return (R[2, 1] - R[1, 2]) / S, 0.25 * S, (R[0, 1] + R[1, 0]) / S, (R[0, 2] + R[2, 0]) / S
    if d[1] > d[2]:
        S = np.sqrt(1.0 + d[1] - d[0] - d[2]) * 2
        return (R[0, 2] - R[2, 0]) / S, (R[0, 1] + R[1, 0]) / S, 0.25 * S, (R[1, 2] + R[2, 1]) / S
    S = np.sqrt(1.0 + d[2] - d[0] - d[1]) * 2
    return (R[1, 0] - R[0, 1]) / S, (R[0, 2] + R[2, 0]) / S, (R[1, 2] + R[2, 1]) / S, 0.25 * S


class SfMExporter:
    """COLMAP text export of a saved reconstruction (export.py:9-187).  Points with fewer than two
    observations are dropped on load, as the reference does."""

    def __init__(self, reconstruction_dir):
        self.recon_dir = Path(reconstruction_dir)
        try:
            self.poses, pts, tracks = load_reconstruction(self.recon_dir, int_keys=False)
        except FileNotFoundError as e:
            raise ValueError(f"Failed to load reconstruction data: {e}")
        self.poses = {k: {'R': R.tolist(), 't': t.ravel().tolist()} for k, (R, t) in self.poses.items()}
        keep = [i for i, tr in enumerate(tracks) if len(tr) >= 2]
        self.points3D = [pts[i] for i in keep]
        self.tracks = [tracks[i] for i in keep]
        logging.info(f"Loaded poses for {len(self.poses)} images, {len(self.points3D)} valid points")

    def export_colmap(self, output_dir):
        output_dir = Path(output_dir)
        output_dir.mkdir(exist_ok=True)
        with open(output_dir / 'cameras.txt', 'w') as f:
            f.write("# Camera list with one line of data per camera:\n"
                    "#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n" + COLMAP_CAMERA_LINE + "\n")
        per_image = {}                       # image id -> ["x y point_id", ...] in point order
        for j, tr in enumerate(self.tracks):
            for img, (x, y) in tr.items():
                per_image.setdefault(img, []).append(f"{x} {y} {j + 1}")
        refs = 0
        with open(output_dir / 'images.txt', 'w') as f:
            f.write("# Image list with two lines of data per image:\n"
                    "#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                    "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
            for img, pose in self.poses.items():
                qw, qx, qy, qz = rotation_to_quaternion(np.array(pose['R']))
                t = np.array(pose['t']).reshape(3)
                obs = per_image.get(str(img), [])
                f.write(f"{img} {qw} {qx} {qy} {qz} {t[0]} {t[1]} {t[2]} 1 {int(img):08d}.jpg\n")
                f.write(" ".join(obs) + "\n")
                refs += len(obs)
        logging.info(f"Total point references in images.txt: {refs}")
        written = 0
        with open(output_dir / 'points3D.txt', 'w') as f:
            f.write("# 3D point list with one line of data per point:\n"
                    "#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
            for j, ((x, y, z), tr) in enumerate(zip(self.points3D, self.tracks)):
                if len(tr) < 2:
                    continue
                views = " ".join(f"{k} 0" for k in sorted(tr.keys()))       # string order, as the reference
                f.write(f"{j + 1} {x} {y} {z} 255 255 255 1.0 {views}\n")
                written += 1
        logging.info(f"Wrote {written} points to points3D.txt")

    def _create_colmap_database(self, db_path):
        """Empty COLMAP database holding the one camera row (export.py:153-187)."""
        db_path = Path(db_path)
        if db_path.exists():
            db_path.unlink()
        conn = sqlite3.connect(db_path)
        try:
            cur = conn.cursor()
            cur.execute("CREATE TABLE cameras (camera_id INTEGER PRIMARY KEY, model INTEGER, width INTEGER, "
                        "height INTEGER, params BLOB)")
            cur.execute("CREATE TABLE images (image_id INTEGER PRIMARY KEY, name TEXT, camera_id INTEGER, "
                        "prior_qw REAL, prior_qx REAL, prior_qy REAL, prior_qz REAL, prior_tx REAL, "
                        "prior_ty REAL, prior_tz REAL)")
            cur.execute("INSERT INTO cameras VALUES (?, ?, ?, ?, ?)",
                        (1, 1, 1024, 768, np.array(COLMAP_CAMERA_PARAMS, dtype=np.float64).tobytes()))
            conn.commit()
        except sqlite3.Error:
            conn.rollback()
            raise
        finally:
            conn.close()

    def export_all(self, output_dir):
        colmap_dir = Path(output_dir) / 'colmap'
        colmap_dir.mkdir(parents=True, exist_ok=True)
        self._create_colmap_database(colmap_dir / 'database.db')
        self.export_colmap(colmap_dir)
        logging.info(f"Exported all formats to {output_dir}")


# --------------------------------------------------------------------------------------------------- PNM
def _pnm_token(data, pos):
    """The next whitespace-delimited header token from `pos`, comments ('#' to the end of the line) skipped."""
    n = len(data)
    while pos < n:
        c = data[pos:pos + 1]
        if c == b"#":
            while pos < n and data[pos:pos + 1] not in (b"\n", b"\r"):
                pos += 1
        elif c.isspace():
            pos += 1
        else:
            break
    start = pos
    while pos < n and not data[pos:pos + 1].isspace() and data[pos:pos + 1] != b"#":
        pos += 1
    if start == pos:
        raise ValueError("truncated PNM header")
    return data[start:pos], pos


def read_pnm(path):
    """A binary PGM (P5) or PPM (P6) with maxval 255 - the reference's silhouettes and images - as [h,w] or [h,w,3] uint8.
    Colour comes back in BGR order, so that the result stands in for cv2.imread.  ValueError for any other file."""
    data = Path(path).read_bytes()
    magic, pos = _pnm_token(data, 0)
    if magic not in (b"P5", b"P6"):
        raise ValueError(f"{path}: not a binary PGM / PPM (magic {magic!r})")
    try:
        w, pos = _pnm_token(data, pos)
        h, pos = _pnm_token(data, pos)
        maxval, pos = _pnm_token(data, pos)
        w, h, maxval = int(w), int(h), int(maxval)
    except ValueError as e:
        raise ValueError(f"{path}: bad PNM header ({e})") from None
    if w < 0 or h < 0 or maxval != 255:
        raise ValueError(f"{path}: only maxval 255 is read (got {w} x {h}, maxval {maxval})")
    pos += 1                                              # the single whitespace byte behind maxval
    ch = 3 if magic == b"P6" else 1
    if len(data) - pos < w * h * ch:
        raise ValueError(f"{path}: truncated: {len(data) - pos} bytes of pixels for {w} x {h} x {ch}")
    a = np.frombuffer(data, dtype=np.uint8, count=w * h * ch, offset=pos)
    return a.reshape(h, w).copy() if ch == 1 else a.reshape(h, w, 3)[:, :, ::-1].copy()


def write_pnm(path, image, comment=None):
    """[h,w] uint8 as P5, [h,w,3] uint8 in BGR order as P6; `comment` goes into the header as a '#' line."""
    a = np.asarray(image)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError("write_pnm takes [h,w] or [h,w,3] uint8")
    head = (b"P5\n" if a.ndim == 2 else b"P6\n") + (b"# " + str(comment).encode() + b"\n" if comment is not None else b"")
    head += f"{a.shape[1]} {a.shape[0]}\n255\n".encode()
    body = a if a.ndim == 2 else a[:, :, ::-1]
    Path(path).write_bytes(head + np.ascontiguousarray(body).tobytes())
