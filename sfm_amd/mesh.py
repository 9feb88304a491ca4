"""A surface from the depth maps on the device: `sfm_tsdf_integrate` (sfm_amd/csrc/tsdf.hip) fills a truncated signed
distance volume from filtered depth maps, `sfm_mesh_mark` / `sfm_mesh_emit` (sfm_amd/csrc/mesh.hip) turn its zero level into
a triangle mesh by marching tetrahedra; include/sfm_amd.h states both rules completely.  Every view weighs the same, a pixel
without a depth carries no evidence (free space outside every silhouette stays unknown and the mesh is open there), holes
are not filled and zero-area triangles are kept.  `sfm_mesh_colors` (sfm_amd/csrc/mesh_color.hip) gives every vertex a colour
blended over the views whose own depth maps see it, `sfm_mesh_texture` (sfm_amd/csrc/mesh_texture.hip) every triangle a
patch of texels in an atlas by the same blend, and `sfm_mesh_render` (sfm_amd/csrc/mesh_render.hip) draws the mesh through
any camera: depth, triangle, barycentrics and colour per pixel; `sfm_render_score` (sfm_amd/csrc/render_score.hip) scores such a
render against the photographs: error, PSNR and SSIM sums and the distance to the views' own depth.  `Mesh.exposure`
(sfm_amd/exposure.py) estimates one gain per view and channel for images whose exposure differs, to be applied before they go
to the colour calls.  `Mesh.components` and `Mesh.clean` (sfm_amd/mesh_clean.py; `sfm_mesh_components`, `sfm_mesh_clean_mark` /
`sfm_mesh_clean_emit`, sfm_amd/csrc/mesh_clean.hip) label the connected components of the mesh and remove the small ones.
`Mesh.decimate` (sfm_amd/mesh_decimate.py; `sfm_mesh_decimate_cluster`, `sfm_mesh_decimate_mark` / `sfm_mesh_decimate_emit`,
sfm_amd/csrc/mesh_decimate.hip) clusters the vertices on a uniform grid and places one vertex per cell by its quadric.
`Mesh.adjacency`, `Mesh.smooth` and `Mesh.recompute_normals` (sfm_amd/mesh_smooth.py; `sfm_mesh_adjacency`, `sfm_mesh_smooth`,
`sfm_mesh_vertex_normals`, sfm_amd/csrc/mesh_smooth.hip) build the neighbours of every vertex, move the vertices by Taubin steps
and re-derive the normals from the faces.  No
CPU fallback: without the library or a GPU the calls raise.
"""
from __future__ import annotations

import ctypes as C
from numbers import Real

import numpy as np

from . import _lib
from ._lib import dp, hp
from ._views import ViewSet, check_color_images, projections_from_backprojections, workspace  # noqa: F401

MIN_DIM, MAX_DIM, MAX_VIEWS = 2, 1024, 65535


def check_grid(origin, voxel, shape):
    """(origin float64 [3], voxel float, (nx, ny, nz)) or ValueError."""
    origin = np.asarray(origin, dtype=np.float64).reshape(-1)
    if origin.shape != (3,) or not np.isfinite(origin).all():
        raise ValueError("origin must be 3 finite numbers")
    if not (isinstance(voxel, Real) and np.isfinite(voxel) and voxel > 0):
        raise ValueError("voxel must be a finite number > 0")
    try:
        shape = tuple(shape)
    except TypeError:
        raise ValueError("shape must be (nx, ny, nz)") from None
    if len(shape) != 3 or any(not (isinstance(n, (int, np.integer)) and MIN_DIM <= n <= MAX_DIM) for n in shape):
        raise ValueError(f"shape must be (nx, ny, nz), integers {MIN_DIM} .. {MAX_DIM}")
    return origin, float(voxel), tuple(int(n) for n in shape)


class Mesh:
    """What `TsdfVolume.mesh` returns; the arrays stay on the device until they are asked for.  vertices float64 [nv,3] in
    (node index, direction) order, normals float32 [nv,3] (unit, pointing to the outside; zeros where the gradient has no
    length), triangles int32 [nt,3] in (cell index, tetrahedron) order, their normals pointing from inside to outside."""

    def __init__(self, state, n_vertices, n_triangles, volume=None):
        self._m = state
        self.n_vertices, self.n_triangles = int(n_vertices), int(n_triangles)
        self._volume = volume                                      # for the defaults of colors(): its truncation, its maps
        self._host = {}

    def _get(self, name, n):
        if name not in self._m:
            return None
        if name not in self._host:
            self._host[name] = self._m[name].cpu().numpy()[:n]
        return self._host[name]

    vertices = property(lambda self: self._get("vertices", self.n_vertices))
    normals = property(lambda self: self._get("normals", self.n_vertices))
    triangles = property(lambda self: self._get("triangles", self.n_triangles))
    # after colors(): uint8 [nv] or [nv,3], uint8 [nv] (the views blended, at most 255), int32 [nv] (-1: no view); None before
    vertex_colors = property(lambda self: self._get("vertex_colors", self.n_vertices))
    n_views = property(lambda self: self._get("n_views", self.n_vertices))
    best_view = property(lambda self: self._get("best_view", self.n_vertices))
    # on what clean() returns: int32 [nv] / [nt], the index each vertex / triangle had in the mesh it was cleaned from; on what
    # decimate() returns: triangle_map alone, likewise; None otherwise
    vertex_map = property(lambda self: self._get("vertex_map", self.n_vertices))
    triangle_map = property(lambda self: self._get("triangle_map", self.n_triangles))
    components_before = None                                       # on what clean() returns: the `MeshComponents` it used

    def components(self):
        """The connected components on the device (`sfm_mesh_components`; include/sfm_amd.h states the rule): vertices are the
        nodes, every triangle joins its three, components are numbered by their smallest vertex.  Returns a `MeshComponents`;
        ValueError when a triangle has an index outside 0 .. nv - 1."""
        from .mesh_clean import components_of
        return components_of(self)

    def clean(self, min_triangles=1, keep_largest=None, components=None):
        """A new `Mesh` without the small components (`sfm_mesh_clean_mark` / `sfm_mesh_clean_emit`): a component stays when
        it has at least min_triangles triangles and, with keep_largest = k, is among the k with the most triangles (equal
        sizes: the lower component number).  components: what `components()` returned for this mesh, None to label it now.
        Kept vertices and triangles keep their order; vertex_colors, n_views and best_view come along when the mesh has them;
        vertex_map and triangle_map give the old indices, components_before the `MeshComponents` used.  The volume is
        carried over, so colors(), texture(), render_views() and score() keep their defaults; atlas is None - its layout is
        a function of the triangle number, so call texture() again.  This mesh is untouched."""
        from .mesh_clean import clean
        return clean(self, min_triangles, keep_largest, components)

    # on what fill_holes() returns: where the new vertices and triangles start, how many sub-loops were filled with how many
    # triangles, how many short sub-loops stayed open, the `MeshEdges` it used; None otherwise
    fill_vertex_start = fill_triangle_start = n_filled = n_fill_triangles = n_open = edges_before = None
    # int32 [n_fill_triangles]: the half-edge of the old mesh that each new triangle closes; None otherwise
    fill_triangle_halfedge = property(lambda self: self._get("fill_triangle_halfedge", self.n_fill_triangles))

    def edges(self):
        """The edge table on the device (`sfm_mesh_edges`; include/sfm_amd.h states the rule): per half-edge 3 t + k how many
        live half-edges use its edge, its twin, the next boundary half-edge about its end and the short boundary loop it is
        on.  Returns a `MeshEdges` with the counts, `is_closed` and `euler`."""
        from .mesh_fill import edges_of
        return edges_of(self)

    def fill_holes(self, max_edges=16, edges=None):
        """A new `Mesh` with the small holes closed (`sfm_mesh_fill_mark` / `sfm_mesh_fill_emit`): every boundary loop of at
        most 64 edges is split where it passes a vertex twice, and every part of 3 .. max_edges edges gets a vertex at the
        mean of its own and one triangle per edge.  edges: what `edges()` returned for this mesh, None to build it now.  The
        old vertices, normals and triangles are byte for byte in front; fill_vertex_start, fill_triangle_start, n_filled,
        n_fill_triangles, fill_triangle_halfedge and edges_before say what was added.  The volume is carried over;
        vertex_colors, n_views, best_view and atlas are None - a new vertex has no colour, so call colors() or texture()
        again.  Longer boundary cycles, an outline among them, stay open; the outline of a lone fragment of at most
        max_edges edges is closed too, so clean() first.  This mesh is untouched."""
        from .mesh_fill import fill_holes
        return fill_holes(self, max_edges, edges)

    # on what smooth() returns: how many vertices the boundary rule and the caller pinned, how many have no neighbour (with
    # n_unsound_vertices: those with a coordinate that is not finite), the `MeshAdjacency` it used; None otherwise
    n_pinned_boundary = n_pinned_given = n_isolated = adjacency_before = None
    # uint8 [nv]: why a vertex stayed (bit 0 boundary, 1 pinned by the caller, 2 not finite, 3 isolated; 0: it moved); None otherwise
    vertex_state = property(lambda self: self._get("vertex_state", self.n_vertices))

    def adjacency(self):
        """The vertex adjacency on the device (`sfm_mesh_adjacency`; include/sfm_amd.h states the rule): per vertex its
        neighbours - the other ends of its live half-edges - in ascending index as ptr / index, and vertex_flags with bit 0
        for a vertex on an edge that is not used exactly twice and bit 1 for one without a neighbour.  Returns a
        `MeshAdjacency` with the counts."""
        from .mesh_smooth import adjacency_of
        return adjacency_of(self)

    def smooth(self, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, pinned=None, normals="recompute", adjacency=None):
        """A new `Mesh` with smoothed vertices (`sfm_mesh_smooth`; include/sfm_amd.h states the rule): every iteration moves
        each free vertex by lam towards the mean of its neighbours and then, unless mu is None, by mu (negative: away) with
        respect to the new mean - Taubin's pair, which keeps the volume that plain Laplacian steps (mu=None) lose.  Boundary
        vertices (pin_boundary), the vertices with pinned[v] != 0 (uint8 / bool [nv]), vertices that are not finite and
        vertices without a neighbour stay; vertex_state says why, n_pinned_boundary, n_pinned_given, n_unsound_vertices and
        n_isolated count them.  normals: "recompute" for area-weighted normals of the moved faces (`sfm_mesh_vertex_normals`),
        "keep" for the old ones.  adjacency: what `adjacency()` returned for this mesh, None to build it now.  The triangles
        are carried over byte for byte and so is the volume; vertex_colors, n_views, best_view and atlas are None, so call
        colors() or texture() again.  iterations=0 returns the vertices byte for byte.  This mesh is untouched."""
        from .mesh_smooth import smooth
        return smooth(self, iterations, lam, mu, pin_boundary, pinned, normals, adjacency)

    def recompute_normals(self):
        """A new `Mesh` with the same vertices and triangles and area-weighted normals (`sfm_mesh_vertex_normals`): the unit
        of the sum of (p1 - p0) x (p2 - p0) over the triangles at each vertex, zeros where that sum has no finite positive
        length.  What a mesh of `decimate_mesh` / `fill_mesh_holes` without normals needs before colors()."""
        from .mesh_smooth import recompute_normals
        return recompute_normals(self)

    # on what decimate() returns: the vertices of the mesh it was made from, how many of them and of its triangles were
    # unsound, how many triangles had two corners in one cell, how many the duplicate rule dropped, the grid; None otherwise
    n_source_vertices = n_unsound_vertices = n_unsound_triangles = n_degenerate = n_cancelled = cell = origin = None
    # int32 [n_source_vertices]: the cluster of each old vertex (-1: unsound); per new vertex int32 its smallest member, int32
    # its member count, uint8 whether the quadric placed it (0: the mean); None otherwise
    vertex_cluster = property(lambda self: self._get("vertex_cluster", self.n_source_vertices))
    cluster_first = property(lambda self: self._get("cluster_first", self.n_vertices))
    cluster_size = property(lambda self: self._get("cluster_size", self.n_vertices))
    cluster_placed = property(lambda self: self._get("cluster_placed", self.n_vertices))

    def decimate(self, cell=None, factor=2.0, origin=None, placement="quadric"):
        """A new `Mesh` with fewer triangles (`sfm_mesh_decimate_cluster`, `sfm_mesh_decimate_mark`, `sfm_mesh_decimate_emit`;
        include/sfm_amd.h states the rule): the vertices are clustered by the cells of a uniform grid of side cell (None:
        factor times the voxel of the mesh's volume) from origin (None: the per-axis minimum of the finite coordinates; the
        extent over cell must then stay below 2^21), every cell becomes one vertex - placement "quadric": where the planes
        of the triangles at the cell meet, kept inside the cell; "mean": the mean of its members -, a triangle stays when its
        vertices land in three cells, and of those on one triple of cells the first of the prevailing orientation, none on a
        tie.  The result carries vertex_cluster, cluster_first, cluster_size, cluster_placed, triangle_map, n_degenerate,
        n_cancelled, n_unsound_vertices, n_unsound_triangles, cell and origin; the volume is carried over; vertex_colors,
        n_views, best_view and atlas are None, so call colors() or texture() again.  Thin features pinch into non-manifold
        edges, which edges() reports; cells that no kept triangle uses stay as vertices until clean().  This mesh is
        untouched."""
        from .mesh_decimate import decimate
        return decimate(self, cell, factor, origin, placement)

    def _views(self, what, maps, images=None, arrays_too=False):
        """The `ViewSet` of a per-view call, with the pixels of images where they are given: that of `maps`, None for the one
        the mesh's volume remembers.  A volume integrated from arrays has no `DepthMaps` behind its set and no centres in
        it; only a caller that says arrays_too takes it."""
        if maps is not None:
            return ViewSet.from_maps(maps, what, images)
        views = getattr(self._volume, "views", None)
        if views is None or (views.maps is None and not arrays_too):
            raise ValueError(f"{what}() needs maps: the mesh's volume was not " + ("integrated from depth maps" if arrays_too else "built by DepthMaps.tsdf()"))
        return views if images is None else views.with_centres().with_images(images)

    def _tol(self, what, tol):
        """tol, None for the truncation of the mesh's volume."""
        if tol is not None:
            return tol
        if self._volume is None:
            raise ValueError(f"{what}() needs tol: the mesh has no volume")
        return getattr(self._volume, "trunc", 3.0 * self._volume.voxel)

    def _view_inputs(self, what, images, maps, tol, min_cos, fill):
        """What colors() and texture() share: the views with their pixels, and tol with its default; both checked."""
        tol = self._tol(what, tol)
        check_color_scalars(tol, min_cos, fill)
        return self._views(what, maps, images), tol

    def colors(self, images, maps=None, tol=None, min_cos=0.35, fill=0):
        """A colour per vertex on the device (`sfm_mesh_colors`; include/sfm_amd.h states the rule): the vertex is projected
        into every view, a view counts when its own depth at the nearest pixel is within tol of the vertex's depth and the
        cosine between the vertex normal and the direction to the camera is at least min_cos, and the bilinear samples of
        the views that count are blended with the weight cos^2.  images: one [h,w] or [h,w,3] uint8 array per IMAGE of the
        set, all with the same channel count, each shaped like its view's maps, channel order untouched; maps: a filtered
        `DepthMaps`, None for those the mesh's volume was integrated from; tol: None for the truncation of the volume
        (3 voxels); fill: the colour of a vertex that no view sees.  Returns uint8 [nv] or [nv,3] and fills vertex_colors,
        n_views and best_view (the position of the view with the largest weight, -1 for none)."""
        views, tol = self._view_inputs("colors", images, maps, tol, min_cos, fill)
        self._m.update(_colors(views, self.n_vertices, self._m["vertices"], self._m["normals"], tol, min_cos, fill))
        for name in ("vertex_colors", "n_views", "best_view"):
            self._host.pop(name, None)
        return self.vertex_colors

    def exposure(self, images, maps=None, tol=None, min_cos=0.35, sigma_n=10.0, sigma_g=1.0, min_overlap=1):
        """One gain per view and channel from the vertices that several views see (`sfm_mesh_exposure_sample`,
        `sfm_mesh_exposure_gram`; include/sfm_amd.h states the rule): every view's sample of every vertex it sees, as
        `colors()` would take it, the counts and sums over the vertices two views share, and the least-squares gains that
        make those sums agree (`solve_gains`; sigma_n the noise of a sample in grey levels, sigma_g how far a gain may stray
        from 1, min_overlap the common vertices a pair needs).  images, maps, tol and min_cos are those of `colors()`; a mesh
        whose volume came from `tsdf_volume_from_depth_arrays` takes one image per view.  Returns an `ExposureGains`; its
        `apply(images)` gives the images to hand to `colors()`, `texture()` and `score()`."""
        from .exposure import mesh_exposure
        return mesh_exposure(self, images, maps, tol, min_cos, sigma_n, sigma_g, min_overlap)

    atlas = None                                                   # the `MeshTexture` of the last texture(); None before

    def texture(self, images, texels=8, maps=None, tol=None, min_cos=0.35, fill=0, cells_per_row=None):
        """A texture atlas on the device (`sfm_mesh_texture`; include/sfm_amd.h states the rule): every triangle gets a patch
        with texels + 1 texel centres along each leg, two triangles to a cell of (texels + 3)^2 texels, cells_per_row cells
        in a row (None: ceil(sqrt(ceil(nt / 2))), a square atlas), and every texel is the blend of `colors()` at the texel's
        point on the triangle, with the normal interpolated from the corners'.  images, maps, tol, min_cos and fill are those
        of `colors()`; fill is also the colour of the texels that belong to no triangle.  Returns a `MeshTexture` and keeps
        it as `atlas`."""
        cells_per_row = check_texture_layout(self.n_triangles, texels, cells_per_row)[0]
        views, tol = self._view_inputs("texture", images, maps, tol, min_cos, fill)
        self.atlas = _texture(views, self.n_vertices, self._m["vertices"], self._m["normals"], self.n_triangles, self._m["triangles"], texels,
                              cells_per_row, tol, min_cos, fill)
        return self.atlas

    def render(self, cameras, sizes, colors="auto", fill=0):
        """The mesh drawn through cameras on the device (`sfm_mesh_render`; include/sfm_amd.h states the rule): per pixel the
        nearest triangle under its centre, its depth, its barycentrics and a colour.  cameras: one [3,4] or [12] projection
        (world to pixels) or a list of them; a camera may also be (K, (R, t)) or (K, R, t), taken as P = K [R | t].  sizes: one
        (width, height) for all cameras or one per camera.  colors: "atlas" samples `atlas` bilinearly at the interpolated uv,
        "vertex" interpolates `vertex_colors`, None draws geometry only, "auto" takes the atlas if the mesh has one, else the
        vertex colours, else none; a source the mesh does not have is a ValueError.  fill: the colour where nothing draws.
        Returns a `MeshRender`."""
        proj, heights, widths = check_render_arguments(cameras, sizes, fill)[:3]
        has_vertex = "vertex_colors" in self._m
        mode = resolve_render_colors(colors, self.atlas is not None, has_vertex)
        vcol = uv = image = None
        channels, size = 1, (0, 0)
        if mode == RENDER_ATLAS:
            image, uv, channels, size = self.atlas._m["image"], self.atlas._m["uv"], self.atlas.channels, self.atlas.size
        elif mode == RENDER_VERTEX:
            vcol = self._m["vertex_colors"]
            channels = 3 if vcol.ndim == 2 else 1
        return _render(self._m["vertices"].device, proj, heights, widths, self.n_vertices, self._m["vertices"], self.n_triangles,
                       self._m["triangles"], mode, channels, vcol, uv, image, size, fill)

    def render_views(self, maps=None, colors="auto", fill=0):
        """`render()` through the cameras of the views of a `DepthMaps`, each at the size of its maps: the render of every
        input photograph that has a depth map.  maps: None for those the mesh's volume was integrated from."""
        maps = self._views("render_views", None).maps if maps is None else maps       # no filter() is needed here
        proj = projections_from_backprojections(maps._s["backproj"].cpu().numpy()[:len(maps.views)])
        return self.render(list(proj), [(w, h) for h, w in maps.shapes], colors, fill)

    def score(self, images, maps=None, colors="auto", **options):
        """`render_views(maps, colors).compare(images, maps, **options)`: every view drawn again and scored against its
        photograph and its own depth map (`sfm_render_score`).  images: one array per IMAGE of the set, as `colors()` and
        `texture()` take them, or one per view; options: masks, window, rel_tol, keep_maps of `MeshRender.compare`.
        Returns a `RenderScore`."""
        maps = self._views("score", None).maps if maps is None else maps
        if len(images) == len(maps._s["imgs"]):
            images = [images[r] for r in maps.views]
        return self.render_views(maps, colors).compare(images, maps, **options)

    def save(self, path, colors=None):
        """Binary PLY with normals (`save_ply_mesh`); colors: None for vertex_colors when `colors()` has made them."""
        from .interchange import save_ply_mesh
        colors = self.vertex_colors if colors is None else colors
        save_ply_mesh(self.vertices, self.triangles, path, normals=self.normals, colors=colors)

    def save_obj(self, path, texture=None):
        """Wavefront OBJ with normals, texture coordinates, a .mtl and the atlas as a .png beside it (`save_obj_mesh`);
        texture: a `MeshTexture`, None for `atlas`.  Three-channel atlases are taken as BGR, like the project's images."""
        from .interchange import save_obj_mesh
        texture = self.atlas if texture is None else texture
        if texture is None:
            raise ValueError("save_obj() needs a texture: call texture() first")
        save_obj_mesh(self.vertices, self.triangles, path, normals=self.normals, uv=texture.uv, texture=texture.image)


class MeshTexture:
    """What `Mesh.texture` returns; the arrays stay on the device until they are asked for.  image uint8 [H,W] or [H,W,3]
    (the channel order of the images), views uint8 [H,W] (the views blended into a texel, at most 255; 0 where no view sees
    it or it belongs to no triangle), uv float32 [nt,3,2]: per triangle corner the centre of its texel as (column, row) over
    (W, H), the row counted downwards from the top; size = (W, H)."""

    def __init__(self, state, size, texels, cells_per_row, channels, n_triangles):
        self._m, self.size, self.texels, self.cells_per_row = state, tuple(size), int(texels), int(cells_per_row)
        self.channels, self.n_triangles = int(channels), int(n_triangles)
        self._host = {}

    def _get(self, name, n, shape):
        if name not in self._host:
            self._host[name] = self._m[name].cpu().numpy().reshape(-1)[:n].reshape(shape)
        return self._host[name]

    @property
    def image(self):
        W, H = self.size
        return self._get("image", H * W * self.channels, (H, W) if self.channels == 1 else (H, W, 3))

    @property
    def views(self):
        W, H = self.size
        return self._get("views", H * W, (H, W))

    @property
    def uv(self):
        return self._get("uv", self.n_triangles * 6, (self.n_triangles, 3, 2))


class TsdfVolume:
    """A truncated signed distance field on a grid of nx x ny x nz nodes, node (i, j, k) at origin + voxel * (i, j, k).
    tsdf float32 and weight uint16, both [nz,ny,nx], stay on the device until they are asked for; origin float64 [3], voxel,
    shape = (nx, ny, nz).  A node without evidence has weight 0 and a NaN tsdf."""

    def __init__(self, tsdf, weight, origin, voxel, shape, min_weight=1):
        self._tsdf, self._weight = tsdf, weight                    # device: float32 [n], int16 [n] holding the uint16 bits
        self.origin, self.voxel, self.shape = origin, voxel, shape
        self.min_weight = min_weight
        self._host = {}

    @property
    def tsdf(self):
        if "tsdf" not in self._host:
            self._host["tsdf"] = self._tsdf.cpu().numpy().reshape(self.shape[::-1])
        return self._host["tsdf"]

    @property
    def weight(self):
        if "weight" not in self._host:
            self._host["weight"] = self._weight.cpu().numpy().view(np.uint16).reshape(self.shape[::-1])
        return self._host["weight"]

    def mesh(self, min_weight=None):
        """The zero level as a `Mesh`.  min_weight: a node counts when at least this many views saw it (None: the volume's
        own, 1 unless `DepthMaps.tsdf` was given another); cells with a node that does not count give no triangle."""
        import torch
        min_weight = self.min_weight if min_weight is None else min_weight
        if not (isinstance(min_weight, (int, np.integer)) and 0 <= min_weight <= 0x7FFFFFFF):
            raise ValueError("min_weight must be an integer >= 0")
        dev = self._tsdf.device
        h = _lib.get_handle(dev.index)
        nx, ny, nz = self.shape
        ws, ws_bytes = workspace(h, dev, "sfm_mesh_workspace_bytes", nx, ny, nz)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        origin = np.ascontiguousarray(self.origin, dtype=np.float64)
        h.call("sfm_mesh_mark", dp(self._tsdf), dp(self._weight), nx, ny, nz, int(min_weight), dp(counts), dp(ws), ws_bytes)
        nv, nt = (int(c) for c in counts.cpu().numpy())            # waits for the mark call: the counts size the outputs
        m = {"vertices": torch.empty((max(nv, 1), 3), dtype=torch.float64, device=dev),
             "normals": torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev),
             "triangles": torch.empty((max(nt, 1), 3), dtype=torch.int32, device=dev)}
        h.call("sfm_mesh_emit", dp(self._tsdf), nx, ny, nz, hp(origin), C.c_double(self.voxel), nv, nt,
               dp(m["vertices"]), dp(m["normals"]), dp(m["triangles"]), dp(ws), ws_bytes)
        m["ws"] = ws                                               # alive until the outputs are: the emit call may still run
        return Mesh(m, nv, nt, self)


def tsdf_volume_from_arrays(tsdf, weight, origin, voxel, device=0):
    """A `TsdfVolume` around a field that was made elsewhere: tsdf (float32) and weight (uint16) are [nz,ny,nx]."""
    import torch
    tsdf = np.ascontiguousarray(tsdf, dtype=np.float32)
    weight = np.ascontiguousarray(weight)
    if tsdf.ndim != 3 or weight.shape != tsdf.shape:
        raise ValueError("tsdf and weight must be [nz,ny,nx] arrays of one shape")
    if weight.dtype.kind not in "iu" or (weight.size and (weight.min() < 0 or weight.max() > 65535)):
        raise ValueError("weight must hold integers 0 .. 65535")
    origin, voxel, shape = check_grid(origin, voxel, tsdf.shape[::-1])
    _lib.get_handle(device)
    dev = torch.device("cuda", device)
    return TsdfVolume(torch.from_numpy(tsdf.reshape(-1)).to(dev), torch.from_numpy(weight.astype(np.uint16).view(np.int16).reshape(-1)).to(dev),
                      origin, voxel, shape)


def bounding_grid(points, resolution=256, margin=0.05):
    """(origin, voxel, shape) of a box around points [n,3]: per axis the 1st to 99th percentile, widened on both sides by
    margin of its length, with cubic voxels so that the longest side has `resolution` nodes."""
    if not (isinstance(resolution, (int, np.integer)) and MIN_DIM <= resolution <= MAX_DIM):
        raise ValueError(f"resolution must be an integer {MIN_DIM} .. {MAX_DIM}")
    if not (isinstance(margin, Real) and margin >= 0):
        raise ValueError("margin must be a number >= 0")
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pts = pts[np.isfinite(pts).all(axis=1)]
    if len(pts) == 0:
        raise ValueError("no kept pixel to put a box around")
    lo, hi = np.percentile(pts, 1, axis=0), np.percentile(pts, 99, axis=0)
    ext = hi - lo
    lo, hi = lo - margin * ext, hi + margin * ext
    longest = float((hi - lo).max())
    if not longest > 0:
        raise ValueError("the kept pixels have no extent")
    voxel = longest / (resolution - 1)
    shape = tuple(int(min(max(np.ceil((hi[a] - lo[a]) / voxel - 1e-9) + 1, MIN_DIM), MAX_DIM)) for a in range(3))
    return lo, voxel, shape


def integrate_depth_maps(maps, origin=None, voxel=None, shape=None, resolution=256, margin=0.05, trunc=None, min_weight=1):
    """What `DepthMaps.tsdf` does."""
    if maps.keep is None:
        raise ValueError("tsdf() needs filter() first")
    given = [a is not None for a in (origin, voxel, shape)]
    if any(given) and not all(given):
        raise ValueError("origin, voxel and shape come together or not at all")
    if not (isinstance(min_weight, (int, np.integer)) and min_weight >= 0):
        raise ValueError("min_weight must be an integer >= 0")
    if len(maps.views) > MAX_VIEWS:
        raise ValueError(f"at most {MAX_VIEWS} views")
    if not all(given):
        kept = [x[k != 0] for x, k in zip(maps.xyz, maps.keep)]
        origin, voxel, shape = bounding_grid(np.concatenate(kept) if kept else np.zeros((0, 3)), resolution, margin)
    origin, voxel, shape = check_grid(origin, voxel, shape)
    trunc = 3.0 * voxel if trunc is None else trunc
    if not (isinstance(trunc, Real) and trunc > 0):
        raise ValueError("trunc must be None or a number > 0")
    vol = _integrate(ViewSet.from_maps(maps, "tsdf"), origin, voxel, shape, trunc)
    vol.min_weight = int(min_weight)
    return vol


def _integrate(views, origin, voxel, shape, trunc):
    """The device call.  The volume remembers the views: what Mesh.colors(), texture(), exposure(), render_views() and score()
    project into by default, and what keeps the call's inputs alive while it may still run."""
    import torch
    dev = views.depth.device
    h = _lib.get_handle(dev.index)
    ws, ws_bytes = workspace(h, dev, "sfm_tsdf_workspace_bytes", views.n_ref)
    n = shape[0] * shape[1] * shape[2]
    tsdf = torch.empty(n, dtype=torch.float32, device=dev)
    weight = torch.empty(n, dtype=torch.int16, device=dev)
    h.call("sfm_tsdf_integrate", *views.args(maps_only=True), hp(origin), C.c_double(voxel), shape[0], shape[1], shape[2],
           C.c_double(float(trunc)), dp(tsdf), dp(weight), dp(ws), ws_bytes)
    vol = TsdfVolume(tsdf, weight, origin, voxel, shape)
    vol.trunc, vol.proj, vol.views, vol._held = float(trunc), views.proj, views, ws
    return vol


def tsdf_volume_from_depth_arrays(proj, depth, keep, origin, voxel, shape, trunc, device=0):
    """A `TsdfVolume` integrated from maps that were made elsewhere: proj float64 [n,12] (row-major [K R | K t]), depth one
    float32 [h,w] per view, keep one uint8 [h,w] per view or None (every finite depth counts)."""
    origin, voxel, shape = check_grid(origin, voxel, shape)
    if not (isinstance(trunc, Real) and trunc > 0):
        raise ValueError("trunc must be a number > 0")
    return _integrate(ViewSet.from_arrays(proj, None, depth, keep, MAX_VIEWS, integration_only=True).to(device), origin, voxel, shape, trunc)


# ------------------------------------------------------------------------------------------- colours
def check_color_scalars(tol, min_cos, fill):
    if not (isinstance(tol, Real) and np.isfinite(tol) and tol >= 0):
        raise ValueError("tol must be a finite number >= 0")
    if not (isinstance(min_cos, Real) and np.isfinite(min_cos) and 0 < min_cos <= 1):
        raise ValueError("min_cos must be a number > 0 and <= 1")
    if not (isinstance(fill, (int, np.integer)) and 0 <= fill <= 255):
        raise ValueError("fill must be an integer 0 .. 255")


def check_mesh_arrays(vertices, normals, triangles=None):
    """(vertices float64 [nv,3], normals float32 [nv,3], triangles int32 [nt,3] or None) of a mesh made elsewhere, or ValueError."""
    vertices = np.ascontiguousarray(vertices, dtype=np.float64)
    normals = np.ascontiguousarray(normals, dtype=np.float32)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or normals.shape != vertices.shape:
        raise ValueError("vertices and normals must be [nv,3]")
    if triangles is None:
        return vertices, normals, None
    tri = np.asarray(triangles)
    if tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu" or (tri.size and (tri.min() < -0x80000000 or tri.max() > 0x7FFFFFFF)):
        raise ValueError("triangles must be [nt,3] integers that fit int32")
    return vertices, normals, np.ascontiguousarray(tri, dtype=np.int32)


def upload_rows(a, dev):
    """[n,3] on the device with one row more: a pointer must exist."""
    import torch
    return torch.from_numpy(np.concatenate([a, np.zeros((1, 3), a.dtype)])).to(dev)


def _colors(views, n_vertices, d_vertices, d_normals, tol, min_cos, fill):
    """The device call: a `ViewSet` with its pixels; the vertices and the normals on the device."""
    import torch
    dev = views.depth.device
    h = _lib.get_handle(dev.index)
    ws, ws_bytes = workspace(h, dev, "sfm_mesh_colors_workspace_bytes", views.n_ref)
    n = max(int(n_vertices), 1)
    out = {"vertex_colors": torch.empty(n if views.channels == 1 else (n, 3), dtype=torch.uint8, device=dev),
           "n_views": torch.empty(n, dtype=torch.uint8, device=dev), "best_view": torch.empty(n, dtype=torch.int32, device=dev)}
    h.call("sfm_mesh_colors", *views.args(), int(n_vertices), dp(d_vertices), dp(d_normals), C.c_double(float(tol)), C.c_double(float(min_cos)),
           int(fill), dp(out["vertex_colors"]), dp(out["n_views"]), dp(out["best_view"]), dp(ws), ws_bytes)
    out["colors_ws"] = (ws,) + views.alive()                       # alive while the call may still run
    return out


def mesh_vertex_colors(vertices, normals, proj, centres, depth, keep, images, tol, min_cos=0.35, fill=0, device=0):
    """`sfm_mesh_colors` on arrays that were made elsewhere: vertices float64 [nv,3], normals float32 [nv,3], proj float64
    [n,12] (row-major [K R | K t]), centres float64 [n,3], depth one float32 [h,w] per view, keep one uint8 [h,w] per view or
    None (every finite depth counts), images one uint8 [h,w] or [h,w,3] per VIEW.  Returns (colors uint8 [nv] or [nv,3],
    n_views uint8 [nv], best_view int32 [nv])."""
    check_color_scalars(tol, min_cos, fill)
    vertices, normals, _ = check_mesh_arrays(vertices, normals)
    views = ViewSet.from_arrays(proj, centres, depth, keep, MAX_VIEWS, images).to(device)
    dev, nv = views.depth.device, len(vertices)
    out = _colors(views, nv, upload_rows(vertices, dev), upload_rows(normals, dev), tol, min_cos, fill)
    return tuple(out[name].cpu().numpy()[:nv] for name in ("vertex_colors", "n_views", "best_view"))


# ------------------------------------------------------------------------------------------- texture
MAX_TEXELS, MAX_ATLAS_SIDE = 64, 32768


def check_texture_layout(n_triangles, texels, cells_per_row):
    """(cells_per_row with None resolved, W, H) of the atlas or ValueError: what `sfm_mesh_texture_size` computes."""
    if not (isinstance(texels, (int, np.integer)) and 1 <= texels <= MAX_TEXELS):
        raise ValueError(f"texels must be an integer 1 .. {MAX_TEXELS}")
    if not 0 <= n_triangles <= 0x7FFFFFFF:
        raise ValueError("at most 2^31 - 1 triangles")
    cells = (int(n_triangles) + 1) // 2
    if cells_per_row is None:
        import math
        r = math.isqrt(cells)
        cells_per_row = max(r + (r * r < cells), 1)
    if not (isinstance(cells_per_row, (int, np.integer)) and cells_per_row >= 1):
        raise ValueError("cells_per_row must be None or an integer >= 1")
    P = int(texels) + 3
    W, H = int(cells_per_row) * P, -(-cells // int(cells_per_row)) * P
    if W > MAX_ATLAS_SIDE or H > MAX_ATLAS_SIDE:
        raise ValueError(f"the atlas would be {W} x {H}: at most {MAX_ATLAS_SIDE} either way (fewer texels, or another cells_per_row)")
    return int(cells_per_row), W, H


def _texture(views, n_vertices, d_vertices, d_normals, n_triangles, d_triangles, texels, cells_per_row, tol, min_cos, fill):
    """The device call: a `ViewSet` with its pixels; the vertices, the normals and the triangles on the device."""
    import torch
    dev, channels = views.depth.device, views.channels
    h = _lib.get_handle(dev.index)
    W, H = C.c_int32(), C.c_int32()
    if h.lib.sfm_mesh_texture_size(int(n_triangles), int(texels), int(cells_per_row), C.byref(W), C.byref(H)) != 0:
        raise ValueError("sfm_mesh_texture_size refuses this layout")
    W, H = W.value, H.value
    ws, ws_bytes = workspace(h, dev, "sfm_mesh_texture_workspace_bytes", views.n_ref)
    out = {"image": torch.empty(max(H * W * channels, 1), dtype=torch.uint8, device=dev),
           "views": torch.empty(max(H * W, 1), dtype=torch.uint8, device=dev),
           "uv": torch.empty(max(int(n_triangles) * 6, 1), dtype=torch.float32, device=dev)}
    h.call("sfm_mesh_texture", *views.args(), int(n_vertices), dp(d_vertices), dp(d_normals), int(n_triangles), dp(d_triangles), int(texels),
           int(cells_per_row), C.c_double(float(tol)), C.c_double(float(min_cos)), int(fill), dp(out["image"]), dp(out["views"]), dp(out["uv"]),
           dp(ws), ws_bytes)
    out["ws"] = (ws, d_vertices, d_normals, d_triangles) + views.alive()       # alive while the call may still run
    return MeshTexture(out, (W, H), texels, cells_per_row, channels, n_triangles)


def mesh_texture(vertices, normals, triangles, proj, centres, depth, keep, images, tol, texels=8, min_cos=0.35, fill=0, cells_per_row=None,
                 device=0):
    """`sfm_mesh_texture` on arrays that were made elsewhere: vertices float64 [nv,3], normals float32 [nv,3], triangles int32
    [nt,3] (a triangle with an index outside 0 .. nv - 1 is seen by no view), the views as `mesh_vertex_colors` takes them,
    images one uint8 [h,w] or [h,w,3] per VIEW.  Returns a `MeshTexture`."""
    check_color_scalars(tol, min_cos, fill)
    vertices, normals, tri = check_mesh_arrays(vertices, normals, triangles)
    cells_per_row = check_texture_layout(len(tri), texels, cells_per_row)[0]
    views = ViewSet.from_arrays(proj, centres, depth, keep, MAX_VIEWS, images).to(device)
    dev = views.depth.device
    return _texture(views, len(vertices), upload_rows(vertices, dev), upload_rows(normals, dev), len(tri), upload_rows(tri, dev), texels,
                    cells_per_row, tol, min_cos, fill)


# ------------------------------------------------------------------------------------------- render
RENDER_NONE, RENDER_VERTEX, RENDER_ATLAS = 0, 1, 2
MAX_CAMERAS, MAX_IMAGE_SIDE = 65535, 32768


def _shape(a):
    """np.shape, None for what has none (a ragged nest)."""
    try:
        return np.shape(a)
    except ValueError:
        return None


def _one_camera(cam):
    """float64 [12] from a [3,4] / [12] projection or from (K, (R, t)) / (K, R, t)."""
    if isinstance(cam, (tuple, list)) and len(cam) in (2, 3) and _shape(cam[0]) == (3, 3):
        K = np.asarray(cam[0], dtype=np.float64)
        R, t = cam[1] if len(cam) == 2 else cam[1:]
        R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(-1)
        if R.shape != (3, 3) or t.shape != (3,):
            raise ValueError("a camera given as K with (R, t) needs R [3,3] and t [3]")
        return (K @ np.c_[R, t]).reshape(12)
    try:
        P = np.asarray(cam, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("a camera must be a [3,4] or [12] projection, or K with (R, t)") from None
    if P.shape not in ((3, 4), (12,)):
        raise ValueError("a camera must be a [3,4] or [12] projection, or K with (R, t)")
    return P.reshape(12)


def check_render_arguments(cameras, sizes, fill=0, vertices=None, triangles=None, vertex_colors=None, uv=None, atlas=None):
    """What `Mesh.render` and `render_mesh` check before the device: (proj float64 [n,12], heights int32 [n], widths int32 [n],
    mode, channels, vertices, triangles, vertex_colors, uv, atlas) or ValueError.  The arrays behind fill are those of
    `render_mesh` and stay None where they are not given."""
    single = (isinstance(cameras, np.ndarray) and cameras.shape in ((3, 4), (12,))) or \
             (isinstance(cameras, (tuple, list)) and len(cameras) in (2, 3) and _shape(cameras[0]) == (3, 3)) or \
             (isinstance(cameras, (tuple, list)) and _shape(cameras) in ((3, 4), (12,)) and _shape(cameras[0]) in ((), (4,)))
    cams = [cameras] if single else list(cameras)
    proj = np.array([_one_camera(c) for c in cams], dtype=np.float64).reshape(-1, 12)
    if len(proj) > MAX_CAMERAS:
        raise ValueError(f"at most {MAX_CAMERAS} cameras")
    whole = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    try:
        pairs = list(sizes)
    except TypeError:
        raise ValueError("sizes must be (width, height) or one such pair per camera") from None
    if len(pairs) == 2 and all(whole(v) for v in pairs):
        pairs = [tuple(pairs)] * len(proj)
    if len(pairs) != len(proj):
        raise ValueError("sizes: one (width, height) for all cameras or one per camera")
    for p in pairs:
        if not (isinstance(p, (tuple, list, np.ndarray)) and len(p) == 2 and all(whole(v) and 0 <= v <= MAX_IMAGE_SIDE for v in p)):
            raise ValueError(f"a size must be (width, height), integers 0 .. {MAX_IMAGE_SIDE}")
    widths = np.array([p[0] for p in pairs], dtype=np.int32)
    heights = np.array([p[1] for p in pairs], dtype=np.int32)
    if not (whole(fill) and 0 <= fill <= 255):
        raise ValueError("fill must be an integer 0 .. 255")
    mode, channels, n_vertices = RENDER_NONE, 1, None
    if vertices is not None:
        vertices = np.ascontiguousarray(vertices, dtype=np.float64)
        if vertices.ndim != 2 or vertices.shape[1] != 3:
            raise ValueError("vertices must be [nv,3]")
        n_vertices = len(vertices)
    if triangles is not None:
        tri = np.asarray(triangles)
        if tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu" or (tri.size and (tri.min() < -0x80000000 or tri.max() > 0x7FFFFFFF)):
            raise ValueError("triangles must be [nt,3] integers that fit int32")
        triangles = np.ascontiguousarray(tri, dtype=np.int32)
    if vertex_colors is not None and (uv is not None or atlas is not None):
        raise ValueError("one source of colour: vertex_colors, or uv with atlas")
    if (uv is None) != (atlas is None):
        raise ValueError("uv and atlas come together")
    if vertex_colors is not None:
        vertex_colors = np.asarray(vertex_colors)
        if vertex_colors.dtype != np.uint8 or vertex_colors.shape not in ((n_vertices,), (n_vertices, 3)):
            raise ValueError("vertex_colors must be uint8 [nv] or [nv,3]")
        mode, channels = RENDER_VERTEX, 3 if vertex_colors.ndim == 2 else 1
        vertex_colors = np.ascontiguousarray(vertex_colors)
    if atlas is not None:
        atlas, uv = np.asarray(atlas), np.asarray(uv)
        nt = 0 if triangles is None else len(triangles)
        if atlas.dtype != np.uint8 or atlas.ndim not in (2, 3) or (atlas.ndim == 3 and atlas.shape[2] != 3):
            raise ValueError("atlas must be uint8 [H,W] or [H,W,3]")
        if nt > 0 and not (1 <= atlas.shape[0] <= MAX_ATLAS_SIDE and 1 <= atlas.shape[1] <= MAX_ATLAS_SIDE):
            raise ValueError(f"the atlas must be 1 .. {MAX_ATLAS_SIDE} wide and high")
        if uv.shape != (nt, 3, 2) or uv.dtype.kind != "f":
            raise ValueError("uv must be a float array [nt,3,2]")
        mode, channels = RENDER_ATLAS, 3 if atlas.ndim == 3 else 1
        atlas, uv = np.ascontiguousarray(atlas), np.ascontiguousarray(uv, dtype=np.float32)
    return proj, heights, widths, mode, channels, vertices, triangles, vertex_colors, uv, atlas


def resolve_render_colors(colors, has_atlas, has_vertex_colors):
    """The colour mode of `Mesh.render` from its `colors` argument and what the mesh has."""
    if colors is None:
        return RENDER_NONE
    if colors == "auto":
        return RENDER_ATLAS if has_atlas else (RENDER_VERTEX if has_vertex_colors else RENDER_NONE)
    if colors == "atlas":
        if not has_atlas:
            raise ValueError('colors="atlas" needs an atlas: call texture() first')
        return RENDER_ATLAS
    if colors == "vertex":
        if not has_vertex_colors:
            raise ValueError('colors="vertex" needs vertex colours: call colors() first')
        return RENDER_VERTEX
    raise ValueError('colors must be "auto", "atlas", "vertex" or None')


class MeshRender:
    """What `Mesh.render` returns; the arrays stay on the device until they are asked for.  Per camera: depth float32 [h,w]
    (NaN where nothing draws), triangle int32 [h,w] (-1 there), bary float32 [h,w,3] (zeros there), color uint8 [h,w] or
    [h,w,3] in the channel order of its source (fill there; None for a render without colour).  sizes = [(width, height)]."""

    def __init__(self, state, heights, widths, channels, has_color):
        self._m, self.channels, self.has_color = state, int(channels), bool(has_color)
        self.sizes = [(int(w), int(h)) for h, w in zip(heights, widths)]
        self._host = {}

    def _split(self, name, tail=()):
        if name not in self._host:
            flat = self._m[name].cpu().numpy().reshape(-1)
            per = int(np.prod(tail, dtype=np.int64)) if tail else 1
            out, o = [], 0
            for w, h in self.sizes:
                out.append(flat[o * per:(o + h * w) * per].reshape((h, w) + tail))
                o += h * w
            self._host[name] = out
        return self._host[name]

    depth = property(lambda self: self._split("depth"))
    triangle = property(lambda self: self._split("triangle"))
    bary = property(lambda self: self._split("bary", (3,)))

    @property
    def color(self):
        if not self.has_color:
            return None
        return self._split("color", () if self.channels == 1 else (3,))

    @property
    def coverage(self):
        """The share of drawn pixels per camera (0 for a camera without a pixel)."""
        return [float((t >= 0).mean()) if t.size else 0.0 for t in self.triangle]

    @property
    def n_large(self):
        """The (camera, triangle) boxes of more than 64 pixels, which the second raster pass drew: the workspace's first word."""
        return int(self._m["ws"][:8].cpu().numpy().view(np.uint64)[0])

    def save_png(self, path, camera=0):
        """The colour image of one camera as a PNG (`write_png`); three channels are taken as BGR and written as RGB, like
        the atlas."""
        from .interchange import write_png
        if not self.has_color:
            raise ValueError("save_png() needs a render with colour")
        image = self.color[camera]
        write_png(path, image[:, :, ::-1] if image.ndim == 3 else image)

    def compare(self, images, maps=None, masks=None, window=7, rel_tol=0.02, keep_maps=True):
        """The render scored against photographs on the device (`sfm_render_score`; include/sfm_amd.h states the rule): per
        camera the absolute and squared error and the SSIM over a uniform window, over the pixels the mesh covers, and how
        far the rendered depth is from the view's own.  images: one uint8 array per camera of the render, shaped like its
        `color`; maps: a filtered `DepthMaps` whose views are the render's cameras, or None for no depth columns; masks:
        None or one uint8 [h,w] array per camera, a pixel is compared where it is > 0; keep_maps: False for the statistics
        alone.  Returns a `RenderScore`."""
        if not self.has_color:
            raise ValueError("compare() needs a render with colour")
        heights = np.array([h for w, h in self.sizes], dtype=np.int32)
        widths = np.array([w for w, h in self.sizes], dtype=np.int32)
        photos, masks = check_score_arguments(heights, widths, self.channels, images, masks, window, rel_tol)
        d_depth = d_keep = None
        if maps is not None:
            if getattr(maps, "keep", None) is None:
                raise ValueError("compare() needs filter() first")
            if [(w, h) for h, w in maps.shapes] != self.sizes:
                raise ValueError("maps: its views must be the render's cameras, each at the size of its maps")
            d_depth, d_keep = maps._s["depth"], maps._s["keep"]
        import torch
        dev = self._m["triangle"].device
        up = lambda a: None if a is None else torch.from_numpy(np.concatenate([a, np.zeros(1, a.dtype)])).to(dev)   # a pointer must exist
        return _score(dev, heights, widths, self.channels, self._m["color"], self._m["triangle"], self._m["depth"], up(photos), up(masks),
                      d_depth, d_keep, window, rel_tol, keep_maps)


def _render(dev, proj, heights, widths, n_vertices, d_vertices, n_triangles, d_triangles, mode, channels, d_vertex_colors, d_uv, d_atlas,
            atlas_size, fill):
    """The device call: proj [n_cam,12], heights and widths (int32) on the host; the mesh and the colour source on the device."""
    import torch
    h = _lib.get_handle(dev.index)
    n_cam = len(heights)
    heights, widths = np.ascontiguousarray(heights, dtype=np.int32), np.ascontiguousarray(widths, dtype=np.int32)
    d_proj = torch.from_numpy(np.ascontiguousarray(proj, dtype=np.float64).reshape(-1, 12)).to(dev) if n_cam else torch.zeros((1, 12), dtype=torch.float64, device=dev)
    hp_some = lambda a: hp(a) if len(a) else None
    ws, ws_bytes = workspace(h, dev, "sfm_mesh_render_workspace_bytes", n_cam, hp_some(heights), hp_some(widths), int(n_vertices), int(n_triangles))
    n_pix = int((heights.astype(np.int64) * widths.astype(np.int64)).sum())
    n = max(n_pix, 1)
    out = {"depth": torch.empty(n, dtype=torch.float32, device=dev), "triangle": torch.empty(n, dtype=torch.int32, device=dev),
           "bary": torch.empty(n * 3, dtype=torch.float32, device=dev)}
    if mode != RENDER_NONE:
        out["color"] = torch.empty(n * channels, dtype=torch.uint8, device=dev)
    h.call("sfm_mesh_render", n_cam, hp_some(heights), hp_some(widths), dp(d_proj), int(n_vertices), dp(d_vertices), int(n_triangles), dp(d_triangles),
           int(mode), int(channels), dp(d_vertex_colors), dp(d_uv), dp(d_atlas), int(atlas_size[0]), int(atlas_size[1]), int(fill),
           dp(out["depth"]), dp(out["triangle"]), dp(out["bary"]), dp(out.get("color")), dp(ws), ws_bytes)
    out["ws"] = ws
    out["held"] = (d_proj, d_vertices, d_triangles, d_vertex_colors, d_uv, d_atlas)         # alive while the call may still run
    return MeshRender(out, heights, widths, channels, mode != RENDER_NONE)


def render_mesh(vertices, triangles, proj, sizes, vertex_colors=None, uv=None, atlas=None, fill=0, device=0):
    """`sfm_mesh_render` on arrays that were made elsewhere: vertices float64 [nv,3], triangles int32 [nt,3] (a triangle with
    an index outside 0 .. nv - 1 draws nothing), proj and sizes as `Mesh.render` takes cameras and sizes, and one source of
    colour or none: vertex_colors uint8 [nv] or [nv,3], or uv float32 [nt,3,2] with atlas uint8 [H,W] or [H,W,3].  Returns
    a `MeshRender`."""
    import torch
    proj, heights, widths, mode, channels, vertices, tri, vcol, uv, atlas = check_render_arguments(
        proj, sizes, fill, vertices, np.zeros((0, 3), np.int32) if triangles is None else triangles, vertex_colors, uv, atlas)
    _lib.get_handle(device)
    dev = torch.device("cuda", device)
    up = lambda a: None if a is None else torch.from_numpy(np.concatenate([a.reshape(-1), np.zeros(1, a.dtype)])).to(dev)      # a pointer must exist
    size = (0, 0) if atlas is None else (atlas.shape[1], atlas.shape[0])
    return _render(dev, proj, heights, widths, len(vertices), up(vertices), len(tri), up(tri), mode, channels, up(vcol), up(uv), up(atlas), size, fill)


# ------------------------------------------------------------------------------------------- score
SCORE_COLUMNS = 16
(SCORE_N_PIXELS, SCORE_N_COMPARED, SCORE_SAD, SCORE_SSE, SCORE_N_SSIM, SCORE_Q_SSIM, SCORE_N_BOTH, SCORE_N_AGREE, SCORE_Q_REL,
 SCORE_N_RENDER_ONLY, SCORE_N_VIEW_ONLY) = (0, 1, 2, 5, 8, 9, 10, 11, 12, 13, 14)
SCORE_Q = 16777216.0                                               # q_ssim and q_rel count in units of 2^-24
MIN_WINDOW, MAX_WINDOW = 3, 11


def score_tile():
    """(width, height) of the tile one workgroup of `sfm_render_score` takes, from the library."""
    w, h = C.c_int32(), C.c_int32()
    if _lib.load().sfm_render_score_tile(C.byref(w), C.byref(h)) != 0:
        raise _lib.SfmError("sfm_render_score_tile failed")
    return w.value, h.value


def check_score_arguments(heights, widths, channels, images, masks=None, window=7, rel_tol=0.02):
    """What `MeshRender.compare` and `score_render` check before the device: (photos uint8 flat, masks uint8 flat or None) or
    ValueError.  heights / widths: the sizes of the render's cameras; images: one uint8 [h,w] (channels 1) or [h,w,3] array per
    camera; masks: None or one uint8 [h,w] array per camera."""
    whole = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    if not (whole(window) and MIN_WINDOW <= window <= MAX_WINDOW and window % 2 == 1):
        raise ValueError(f"window must be an odd integer {MIN_WINDOW} .. {MAX_WINDOW}")
    if not (isinstance(rel_tol, Real) and not isinstance(rel_tol, bool) and np.isfinite(rel_tol) and rel_tol >= 0):
        raise ValueError("rel_tol must be a finite number >= 0")
    n = len(heights)
    if n > MAX_CAMERAS:
        raise ValueError(f"at most {MAX_CAMERAS} views")
    if any(not (0 <= int(v) <= MAX_IMAGE_SIDE) for v in list(heights) + list(widths)):
        raise ValueError(f"every image side must be 0 .. {MAX_IMAGE_SIDE}")

    def flat(arrays, what, tail):
        try:
            arrays = list(arrays)
        except TypeError:
            raise ValueError(f"{what}: one array per camera of the render") from None
        if len(arrays) != n:
            raise ValueError(f"{what}: one array per camera of the render")
        out = []
        for a, h, w in zip(arrays, heights, widths):
            a = np.asarray(a)
            if a.dtype != np.uint8 or a.shape != (int(h), int(w)) + tail:
                raise ValueError(f"{what}: every array must be uint8 {['h', 'w'] + list(tail)}, shaped like the render")
            out.append(np.ascontiguousarray(a).reshape(-1))
        return np.concatenate(out) if out else np.zeros(0, np.uint8)

    photos = flat(images, "images", () if channels == 1 else (3,))
    return photos, None if masks is None else flat(masks, "masks", ())


def score_figures(stats, channels):
    """The figures of one row of the table, or of the sum of several rows, formed in double from the integers: dict(n_compared,
    mae [c], mse [c], psnr, ssim, n_ssim, depth_both, depth_agree, depth_rel, render_only, view_only).  A mean over nothing is
    NaN; PSNR = 10 log10(255^2 n_compared c / sum sse) is inf for a squared error of 0."""
    import math
    s = [int(v) for v in np.asarray(stats, dtype=np.int64).reshape(-1, SCORE_COLUMNS).sum(0)]
    n = s[SCORE_N_COMPARED]
    div = lambda a, b: a / b if b else float("nan")
    sse = sum(s[SCORE_SSE:SCORE_SSE + channels])
    psnr = float("nan") if n == 0 else (float("inf") if sse == 0 else 10.0 * math.log10(65025.0 * n * channels / sse))
    return dict(n_compared=n, mae=[div(s[SCORE_SAD + k], n) for k in range(channels)], mse=[div(s[SCORE_SSE + k], n) for k in range(channels)],
                psnr=psnr, ssim=div(s[SCORE_Q_SSIM], SCORE_Q * s[SCORE_N_SSIM]), n_ssim=s[SCORE_N_SSIM], depth_both=s[SCORE_N_BOTH],
                depth_agree=div(s[SCORE_N_AGREE], s[SCORE_N_BOTH]), depth_rel=div(s[SCORE_Q_REL], SCORE_Q * s[SCORE_N_BOTH]),
                render_only=s[SCORE_N_RENDER_ONLY], view_only=s[SCORE_N_VIEW_ONLY])


class RenderScore:
    """What `MeshRender.compare` returns; the arrays stay on the device until they are asked for.  stats int64 [n,16] is the
    table of `sfm_render_score`; per view from it: n_compared, mae and mse float64 [n,c], psnr, ssim (NaN without a window),
    n_ssim, depth_both, depth_agree (the share of depth_both within rel_tol), depth_rel (the mean relative difference, each
    capped at 1), render_only, view_only.  abs_error uint8 [h,w] or [h,w,3] and ssim_map float32 [h,w] (NaN without a window)
    per view; None when the maps were not kept."""

    def __init__(self, state, heights, widths, channels, window, rel_tol, has_maps):
        self._m, self.channels, self.window, self.rel_tol, self.has_maps = state, int(channels), int(window), float(rel_tol), bool(has_maps)
        self.sizes = [(int(w), int(h)) for h, w in zip(heights, widths)]
        self._host = {}

    _split = MeshRender._split

    @property
    def stats(self):
        if "stats" not in self._host:
            self._host["stats"] = self._m["stats"].cpu().numpy().reshape(-1)[:len(self.sizes) * SCORE_COLUMNS].reshape(-1, SCORE_COLUMNS)
        return self._host["stats"]

    @property
    def abs_error(self):
        return self._split("abs_error", () if self.channels == 1 else (3,)) if self.has_maps else None

    @property
    def ssim_map(self):
        return self._split("ssim_map") if self.has_maps else None

    def _figures(self):
        if "figures" not in self._host:
            self._host["figures"] = [score_figures(row, self.channels) for row in self.stats]
        return self._host["figures"]

    def _column(self, name, dtype):
        return np.array([f[name] for f in self._figures()], dtype=dtype).reshape((len(self.sizes),) + ((self.channels,) if name in ("mae", "mse") else ()))

    n_compared = property(lambda self: self._column("n_compared", np.int64))
    mae = property(lambda self: self._column("mae", np.float64))
    mse = property(lambda self: self._column("mse", np.float64))
    psnr = property(lambda self: self._column("psnr", np.float64))
    ssim = property(lambda self: self._column("ssim", np.float64))
    n_ssim = property(lambda self: self._column("n_ssim", np.int64))
    depth_both = property(lambda self: self._column("depth_both", np.int64))
    depth_agree = property(lambda self: self._column("depth_agree", np.float64))
    depth_rel = property(lambda self: self._column("depth_rel", np.float64))
    render_only = property(lambda self: self._column("render_only", np.int64))
    view_only = property(lambda self: self._column("view_only", np.int64))

    def pooled(self):
        """The figures of all views together (`score_figures` of the summed integers, not a mean of the views' figures)."""
        return score_figures(self.stats, self.channels)

    def worst(self, k=5, by="ssim"):
        """The positions of the k worst views: the lowest ssim, psnr or depth_agree, the highest mae (mean over the channels)
        or depth_rel; a view without a figure (NaN) comes last."""
        if by not in ("ssim", "psnr", "mae", "depth_agree", "depth_rel"):
            raise ValueError('by must be "ssim", "psnr", "mae", "depth_agree" or "depth_rel"')
        v = getattr(self, by)
        v = v.mean(axis=1) if by == "mae" else v
        key = -v if by in ("mae", "depth_rel") else v
        order = np.argsort(np.where(np.isnan(key), np.inf, key), kind="stable")
        return [int(i) for i in order[:max(int(k), 0)]]

    def save_png(self, path, camera=0, what="error"):
        """One view's map as a PNG (`write_png`): what="error" writes abs_error (three channels are taken as BGR and written as
        RGB, like the render), what="ssim" writes ssim_map mapped linearly from [-1, 1] to 0 .. 255, NaN to 0."""
        from .interchange import write_png
        if not self.has_maps:
            raise ValueError("save_png() needs the maps: compare(..., keep_maps=True)")
        if what == "error":
            image = self.abs_error[camera]
            write_png(path, image[:, :, ::-1] if image.ndim == 3 else image)
        elif what == "ssim":
            write_png(path, ssim_to_gray(self.ssim_map[camera]))
        else:
            raise ValueError('what must be "error" or "ssim"')


def ssim_to_gray(ssim_map):
    """uint8 from an SSIM map: floor((s + 1) * 127.5 + 0.5) cut to 0 .. 255, NaN to 0."""
    s = np.asarray(ssim_map, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        g = np.clip(np.floor((s + 1.0) * 127.5 + 0.5), 0.0, 255.0)
    return np.where(np.isnan(s), 0.0, g).astype(np.uint8)


def _score(dev, heights, widths, channels, d_color, d_triangle, d_depth, d_photos, d_masks, d_view_depth, d_view_keep, window, rel_tol, keep_maps):
    """The device call: heights and widths (int32) on the host, everything else on the device, views back to back."""
    import torch
    h = _lib.get_handle(dev.index)
    n_view = len(heights)
    heights, widths = np.ascontiguousarray(heights, dtype=np.int32), np.ascontiguousarray(widths, dtype=np.int32)
    hp_some = lambda a: hp(a) if len(a) else None
    ws, ws_bytes = workspace(h, dev, "sfm_render_score_workspace_bytes", n_view, hp_some(heights), hp_some(widths))
    n = max(int((heights.astype(np.int64) * widths.astype(np.int64)).sum()), 1)
    out = {"stats": torch.empty(max(n_view, 1) * SCORE_COLUMNS, dtype=torch.int64, device=dev)}
    if keep_maps:
        out["abs_error"] = torch.empty(n * channels, dtype=torch.uint8, device=dev)
        out["ssim_map"] = torch.empty(n, dtype=torch.float32, device=dev)
    h.call("sfm_render_score", n_view, hp_some(heights), hp_some(widths), int(channels), dp(d_color), dp(d_triangle), dp(d_depth), dp(d_photos), dp(d_masks),
           dp(d_view_depth), dp(d_view_keep), int(window), C.c_double(float(rel_tol)), dp(out["stats"]), dp(out.get("abs_error")),
           dp(out.get("ssim_map")), dp(ws), ws_bytes)
    out["held"] = (ws, d_color, d_triangle, d_depth, d_photos, d_masks, d_view_depth, d_view_keep)        # alive while the call may still run
    return RenderScore(out, heights, widths, channels, window, rel_tol, keep_maps)


def score_render(color, triangle, depth, photos, view_depth=None, view_keep=None, masks=None, window=7, rel_tol=0.02, device=0):
    """`sfm_render_score` on arrays that were made elsewhere: per view color uint8 [h,w] or [h,w,3], triangle int32 [h,w] and
    depth float32 [h,w] as a render holds them, photos shaped like color; view_depth float32 [h,w] with view_keep uint8 [h,w]
    per view (both or neither; view_keep None with view_depth keeps every pixel), masks uint8 [h,w].  Returns a `RenderScore`."""
    import torch
    try:
        color = [np.asarray(c) for c in color]
    except TypeError:
        raise ValueError("color: one array per view") from None
    if any(c.dtype != np.uint8 or c.ndim not in (2, 3) or (c.ndim == 3 and c.shape[2] != 3) for c in color) or len({c.ndim for c in color}) > 1:
        raise ValueError("color: uint8 [h,w] or [h,w,3] arrays, all with the same channel count")
    channels = 3 if (color and color[0].ndim == 3) else 1
    heights = np.array([c.shape[0] for c in color], dtype=np.int32)
    widths = np.array([c.shape[1] for c in color], dtype=np.int32)
    flat_photos, flat_masks = check_score_arguments(heights, widths, channels, photos, masks, window, rel_tol)
    if view_depth is None and view_keep is not None:
        raise ValueError("view_keep comes with view_depth")

    def flat(arrays, what, dtype):
        arrays = list(arrays)
        if len(arrays) != len(color) or any(np.shape(a) != (h, w) for a, h, w in zip(arrays, heights, widths)):
            raise ValueError(f"{what}: one [h,w] array per view, shaped like the render")
        return np.concatenate([np.ascontiguousarray(a, dtype=dtype).reshape(-1) for a in arrays] + [np.zeros(1, dtype)])

    tri, dr = flat(triangle, "triangle", np.int32), flat(depth, "depth", np.float32)
    vd = vk = None
    if view_depth is not None:
        vd = flat(view_depth, "view_depth", np.float32)
        vk = np.ones(len(vd), np.uint8) if view_keep is None else flat(view_keep, "view_keep", np.uint8)
    _lib.get_handle(device)
    dev = torch.device("cuda", device)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    pad = lambda a: None if a is None else np.concatenate([a, np.zeros(1, a.dtype)])                          # a pointer must exist
    col = pad(np.concatenate([c.reshape(-1) for c in color]) if color else np.zeros(0, np.uint8))
    return _score(dev, heights, widths, channels, up(col), up(tri), up(dr), up(pad(flat_photos)), up(pad(flat_masks)), up(vd), up(vk), window, rel_tol, True)


from .mesh_clean import MeshComponents, check_clean_arguments, clean_mesh, mesh_components  # noqa: E402,F401
from .mesh_fill import MeshEdges, check_fill_arguments, fill_mesh_holes, mesh_edges  # noqa: E402,F401
from .mesh_decimate import check_decimate_arguments, decimate_mesh  # noqa: E402,F401
from .mesh_smooth import MeshAdjacency, check_smooth_arguments, mesh_adjacency, mesh_vertex_normals, smooth_mesh  # noqa: E402,F401
