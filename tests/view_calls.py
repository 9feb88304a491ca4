"""The view arguments of sfm_tsdf_integrate, sfm_mesh_colors, sfm_mesh_texture and sfm_mesh_exposure_sample for the tests that
hand them bad calls: one good set, the cases tsdf_check_views must refuse, and the calls in which every pointer that has
nothing behind it is null.  Each test keeps its own call, its scalars and the names of its other pointers."""
import ctypes as C

import numpy as np

i32 = lambda *v: np.array(v, dtype=np.int32)
hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
ONE = C.c_void_p(1)                                                # stands for a pointer that is there; never followed

# two images of 3 x 4 and 4 x 7, both views, in swapped order; keep may always be null
GOOD = dict(hs=i32(3, 4), ws=i32(4, 7), n_img=2, n_ref=2, refs=i32(1, 0), proj=ONE, centres=ONE, depth=ONE, keep=None, pixels=ONE)
VIEW_POINTERS = ("proj", "centres", "depth", "pixels")

# refused with a reason of their own: a negative size, a reference out of range (above, below), one listed twice, more views
# than images, a negative count of views, more than 65,535 views, a negative count of images
BAD_SIZES = [dict(hs=i32(3, -1)), dict(refs=i32(0, 2)), dict(refs=i32(-1, 0)), dict(refs=i32(1, 1)), dict(n_ref=3), dict(n_ref=-1),
             dict(n_ref=65536, n_img=65536), dict(n_img=-1)]
# refused as null pointers
NULL_ARRAYS = [dict(hs=None), dict(refs=None)]
BAD_VIEWS = BAD_SIZES + NULL_ARRAYS

# fine when the call has nothing to do: no view at all, and views without a pixel
NO_VIEW = dict(n_ref=0, n_img=0, hs=None, ws=None, refs=None, proj=None, centres=None, depth=None, pixels=None)
NO_PIXEL = dict(hs=i32(0, 4), ws=i32(4, 0), depth=None, pixels=None)
