"""ctypes binding of libsid_pm.so (the C ABI of include/sid_pm.h).

This is the only way the Python host code reaches the GPU.  There is no CPU fallback:
if the HIP library is missing or no gfx950 device is visible, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SID_PM_LIB') or os.path.join(_HERE, 'libsid_pm.so')   # SID_PM_LIB: A/B builds

HES_NORM = 1
HES_SMTH = 2
MCC_NORM = 4
ROT_ORDER1 = 8          # rot_order=1: bilinear template sampling (include/sid_pm.h)
SUBPIXEL = 128          # subpixel=True: parabolic sub-pixel peak (SID_PM_SUBPIXEL; not the reference's)

ABI_VERSION = 6

# every symbol include/sid_pm.h declares
SYMBOLS = (
    'sid_pm_abi_version', 'sid_pm_strerror', 'sid_pm_last_error', 'sid_pm_device_count',
    'sid_pm_batch', 'sid_pm_create', 'sid_pm_destroy', 'sid_pm_set_stream', 'sid_pm_upload_pair',
    'sid_pm_select_pair', 'sid_pm_bind_pair', 'sid_pm_set_points', 'sid_pm_bind_results', 'sid_pm_run', 'sid_pm_sync', 'sid_pm_check', 'sid_pm_unpermute',
    'sid_pm_fetch', 'sid_pm_device_results', 'sid_pm_work_info', 'sid_pm_debug_point', 'sid_pm_debug_ncc_selftest',
    'sid_pm_debug_rsqrt', 'sid_pm_debug_hypot_selftest', 'sid_pm_estimate_cost', 'sid_pm_estimate_residency',
    'sid_pm_rotate_and_match', 'sid_pm_get_template', 'sid_pm_get_hessian', 'sid_pm_estimate_run_time',
)

# every symbol include/sid_ft.h declares (feature-tracking matcher, same library)
FT_SYMBOLS = ('sid_ft_knn2', 'sid_ft_knn2_device', 'sid_ft_workspace_bytes', 'sid_ft_debug_plan', 'sid_ft_last_error', 'sid_ft_release')

# every symbol include/sid_stage.h declares (uint8 staging, same library)
STAGE_SYMBOLS = ('sid_stage_create', 'sid_stage_destroy', 'sid_stage_begin', 'sid_stage_begin_hint', 'sid_stage_order_stats_ws',
                 'sid_stage_count_valid', 'sid_stage_order_stats', 'sid_stage_scale_u8', 'sid_stage_debug_route',
                 'sid_stage_last_error')

# every symbol include/sid_orb.h declares (key-point detector, same library)
ORB_SYMBOLS = ('sid_orb_detect', 'sid_orb_last_error', 'sid_orb_release')

# every symbol include/sid_fg.h declares (first-guess evaluation, same library)
FG_SYMBOLS = ('sid_fg_interp_linear', 'sid_fg_nearest_dist', 'sid_fg_distance_image', 'sid_fg_knn', 'sid_fg_debug_route', 'sid_fg_last_error',
              'sid_fg_release')

# every symbol include/sid_defor.h declares (deformation on a triangulation, same library)
DEFOR_SYMBOLS = ('sid_defor_triangulation', 'sid_defor_elems', 'sid_defor_triangulation_device', 'sid_defor_elems_device',
                 'sid_defor_debug_hypot', 'sid_defor_last_error', 'sid_defor_release')
DEFOR_ERR_INDEX = -32   # include/sid_defor.h SID_DEFOR_ERR_INDEX
# every symbol include/sid_grid.h declares (outlier filter and deformation on a grid of drift vectors, same library)
GRID_SYMBOLS = ('sid_grid_filter', 'sid_grid_deformation', 'sid_grid_filter_device', 'sid_grid_deformation_device',
                'sid_grid_fill', 'sid_grid_smooth', 'sid_grid_fill_device', 'sid_grid_smooth_device',
                'sid_grid_last_error', 'sid_grid_release')
GRID_DIAGONALS = {'shorter': 0, 'main': 1, 'anti': 2}     # SID_GRID_DIAG_*
GRID_TILE = (8, 32)                                       # SID_GRID_TILE_ROWS, SID_GRID_TILE_COLS: the filter kernel's tile
# include/sid_warp.h: piecewise-affine warp of an image along a drift grid
WARP_SYMBOLS = ('sid_warp_image', 'sid_warp_image_device', 'sid_warp_last_error', 'sid_warp_release')
WARP_DTYPES = {'uint8': 0, 'float32': 1}                  # SID_WARP_U8, SID_WARP_F32
WARP_KEEP_ZERO = 1                                        # SID_WARP_KEEP_ZERO
WARP_TILE = (16, 64)                                      # SID_WARP_TILE_ROWS, SID_WARP_TILE_COLS: one work item of the warp kernel
# include/sid_corr.h: local correlation of two uint8 images
CORR_SYMBOLS = ('sid_corr_lattice', 'sid_corr_points', 'sid_corr_lattice_device', 'sid_corr_points_device', 'sid_corr_last_error',
                'sid_corr_release')
CORR_TILE = (8, 64)                                       # SID_CORR_TILE_ROWS, SID_CORR_TILE_COLS: the nodes of one workgroup
# include/sid_track.h: arbitrary points mapped through a drift grid
TRACK_SYMBOLS = ('sid_track_points', 'sid_track_points_device', 'sid_track_last_error', 'sid_track_release')
TRACK_CLOSED = 1                                          # SID_TRACK_CLOSED
TRACK_BRUTE_CELLS = 64                                    # SID_TRACK_BRUTE_CELLS: grids below it look at every cell for every point
# include/sid_ftg.h: guided feature matching, Hamming k=2 within a search radius
FTG_SYMBOLS = ('sid_ftg_knn2', 'sid_ftg_knn2_device', 'sid_ftg_workspace_bytes', 'sid_ftg_debug_plan', 'sid_ftg_last_error',
               'sid_ftg_release')
FTG_MAX_TRAIN = 1 << 22                                   # the index bits of the ordering key: n2 below it

# every symbol include/sid_prep.h declares (sigma0 preparation: dB, HH correction, mask, detrend; same library)
PREP_SYMBOLS = ('sid_prep_subsample', 'sid_prep_apply', 'sid_prep_spatial_mean', 'sid_prep_debug_log10', 'sid_prep_last_error')

# every symbol include/sid_mask.h declares (the invalid-pixel mask: zoomed water mask OR non-finite pixels; same library)
MASK_SYMBOLS = ('sid_mask_workspace_bytes', 'sid_mask_landmask', 'sid_mask_invalid', 'sid_mask_last_error')

# every symbol include/sid_resize.h declares (downsampling by area average, alone and as the front of the preparation; same library)
RESIZE_SYMBOLS = ('sid_resize_f32', 'sid_resize_u8', 'sid_resize_prep_apply', 'sid_resize_prep_subsample', 'sid_resize_last_error')
RESIZE_MAX_DIM = 1 << 24                                  # SID_RESIZE_MAX_DIM

_u8p = C.POINTER(C.c_uint8)
_f64p = C.POINTER(C.c_double)
_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_lib = None


class SidPmError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, 'sid_pm error %d: %s' % (code, msg))
        self.code = code


def lib():
    """Load libsid_pm.so once; raise with build instructions if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            '%s not found: build it with `make -C %s` (hipcc --offload-arch=gfx950) or '
            '`python -c "import __graft_entry__ as g; g.build()"`. There is no CPU fallback.'
            % (LIB_PATH, os.path.join(_HERE, 'csrc')))
    try:                                      # torch first: its wheel carries its own HIP runtime (same soname), and the
        import torch                          # process must end up with one copy - torch cannot enumerate the GPU after
        if torch.cuda.is_available():         # the system runtime has initialised it ("No HIP GPUs are available")
            torch.cuda.init()
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    img = [_u8p, C.c_int64, C.c_int64, C.c_int64]
    ptr = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
    L.sid_pm_abi_version.restype = C.c_int
    L.sid_pm_strerror.restype = C.c_char_p
    L.sid_pm_strerror.argtypes = [C.c_int]
    L.sid_pm_last_error.restype = C.c_char_p
    L.sid_pm_device_count.argtypes = [C.POINTER(C.c_int)]
    L.sid_pm_batch.argtypes = img + img + [_f64p] * 5 + [C.c_int64, C.c_int, C.c_double, _f64p, _f64p,
                                                        C.c_int, C.c_uint32, _f64p, _i32p]
    L.sid_pm_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.sid_pm_destroy.argtypes = [C.c_void_p]
    L.sid_pm_destroy.restype = None
    L.sid_pm_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.sid_pm_upload_pair.argtypes = [C.c_void_p, C.c_int] + img + img
    L.sid_pm_select_pair.argtypes = [C.c_void_p, C.c_int]
    L.sid_pm_bind_pair.argtypes = [C.c_void_p] + ptr + ptr
    L.sid_pm_set_points.argtypes = [C.c_void_p] + [_f64p] * 5 + [C.c_int64, C.c_int, C.c_double, _f64p, _f64p,
                                                                C.c_int, C.c_uint32]
    L.sid_pm_bind_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.sid_pm_run.argtypes = [C.c_void_p]
    L.sid_pm_sync.argtypes = [C.c_void_p]
    if hasattr(L, 'sid_pm_check'):               # (absent from the libraries of earlier rounds that A/B runs load through SID_PM_LIB)
        L.sid_pm_check.argtypes = [C.c_void_p]
    L.sid_pm_fetch.argtypes = [C.c_void_p, _f64p, _i32p]
    L.sid_pm_device_results.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.sid_pm_work_info.argtypes = [C.c_void_p, _f64p]
    L.sid_pm_debug_point.argtypes = [C.c_void_p] + [C.c_double] * 5 + [C.c_int, C.c_double, _f64p, _f64p, C.c_int,
                                                                      C.c_uint32, _u8p, _f32p, _f32p, C.c_int64,
                                                                      _i32p, _f64p, _i32p, C.POINTER(C.c_int64)]
    L.sid_pm_debug_rsqrt.argtypes = [C.c_void_p, _f64p, _f64p, C.c_int64]
    L.sid_pm_debug_ncc_selftest.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_int, C.POINTER(C.c_uint64)]
    if hasattr(L, 'sid_pm_unpermute'):
        L.sid_pm_unpermute.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sid_pm_estimate_cost.argtypes = [_f64p, C.c_int64, C.c_int, C.c_int, C.c_uint32, _f64p]
    L.sid_pm_estimate_residency.argtypes = [_f64p, C.c_int64, C.c_int, C.c_int, C.c_uint32, _i32p]
    L.sid_pm_debug_hypot_selftest.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(C.c_uint64)]
    if hasattr(L, 'sid_pm_estimate_run_time'):
        L.sid_pm_estimate_run_time.argtypes = [_f64p, C.c_int64, C.c_int, C.c_int, C.c_uint32, _f64p]
    if hasattr(L, 'sid_pm_rotate_and_match'):
        L.sid_pm_rotate_and_match.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                              C.c_double, _f64p, _f64p, C.c_int, C.c_uint32, _f64p, _i32p, _f32p, C.c_int64, _u8p]
        L.sid_pm_get_template.argtypes = [C.c_int, _u8p, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double, _f64p, C.c_int, C.c_int, _u8p]
        L.sid_pm_get_hessian.argtypes = [C.c_int, _f32p, C.c_int64, C.c_int64, C.c_uint32, _f32p]
    L.sid_ft_knn2.argtypes = [C.c_int, _u8p, C.c_int64, _u8p, C.c_int64, _i32p, _i32p]
    L.sid_ft_knn2_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sid_ft_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
    L.sid_ft_workspace_bytes.restype = C.c_int64
    L.sid_ft_last_error.restype = C.c_char_p
    if hasattr(L, 'sid_ft_debug_plan'):          # (absent from the libraries of earlier rounds that A/B runs load through SID_PM_LIB)
        L.sid_ft_debug_plan.argtypes = [C.c_int64, C.c_int64, C.c_void_p]
    L.sid_stage_count_valid.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]
    L.sid_stage_order_stats.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_int,
                                        _f32p, C.c_void_p]
    L.sid_stage_scale_u8.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_void_p,
                                     C.c_int64, C.c_void_p]
    L.sid_stage_last_error.restype = C.c_char_p
    L.sid_stage_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.sid_stage_destroy.argtypes = [C.c_void_p]
    L.sid_stage_destroy.restype = None
    L.sid_stage_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]
    L.sid_stage_order_stats_ws.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int, _f32p]
    if hasattr(L, 'sid_stage_begin_hint'):
        L.sid_stage_begin_hint.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_double), C.c_int,
                                           C.POINTER(C.c_int64), C.c_void_p]
    if hasattr(L, 'sid_stage_debug_route'):      # (absent from the libraries of earlier rounds that A/B runs load through SID_PM_LIB)
        L.sid_stage_debug_route.argtypes = [C.c_void_p, C.c_void_p]
    L.sid_orb_detect.argtypes = [C.c_int, _u8p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int8), _i32p,
                                 _f32p, _i32p, C.POINTER(C.c_int64), _u8p, C.c_int64, C.POINTER(C.c_int64)]
    L.sid_orb_last_error.restype = C.c_char_p
    L.sid_fg_interp_linear.argtypes = [C.c_int, _f64p, C.c_int64, _i32p, C.c_int64, _f64p, _f64p, C.c_int64, _f64p, _i32p, _i32p]
    L.sid_fg_nearest_dist.argtypes = [C.c_int, _f64p, C.c_int64, _f64p, C.c_int64, _f64p]
    if hasattr(L, 'sid_fg_distance_image'):
        L.sid_fg_distance_image.argtypes = [C.c_int, _f64p, C.c_int64, C.c_int64, C.c_int64, _f64p]
    if hasattr(L, 'sid_fg_knn'):                 # (absent from the libraries of earlier rounds that A/B runs load through SID_PM_LIB)
        L.sid_fg_knn.argtypes = [C.c_int, _f64p, C.c_int64, _f64p, _f64p, C.c_int64, C.c_int, C.c_double, _f64p, _i32p, _i32p]
    L.sid_fg_last_error.restype = C.c_char_p
    if hasattr(L, 'sid_fg_debug_route'):         # (absent from the libraries of earlier rounds that A/B runs load through SID_PM_LIB)
        L.sid_fg_debug_route.argtypes = [C.c_void_p]
    if hasattr(L, 'sid_defor_triangulation'):
        vp = C.c_void_p
        L.sid_defor_triangulation.argtypes = [C.c_int] + [_f64p] * 4 + [C.c_int64, vp, C.c_int, C.c_int64] + [_f64p] * 5
        L.sid_defor_elems.argtypes = [C.c_int] + [_f64p] * 5 + [C.c_int64] + [_f64p] * 3
        L.sid_defor_triangulation_device.argtypes = [vp] * 4 + [C.c_int64, vp, C.c_int, C.c_int64] + [vp] * 5 + [vp]
        L.sid_defor_elems_device.argtypes = [vp] * 5 + [C.c_int64] + [vp] * 3 + [vp]
        L.sid_defor_debug_hypot.argtypes = [C.c_int, _f64p, _f64p, C.c_int64, _f64p]
        L.sid_defor_last_error.restype = C.c_char_p
        L.sid_defor_release.argtypes = [C.c_int]
    if hasattr(L, 'sid_grid_filter'):
        vp = C.c_void_p
        flt = [C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int, C.c_int]
        L.sid_grid_filter.argtypes = [C.c_int, _f64p, _f64p, _u8p] + flt + [_u8p, _f64p]
        L.sid_grid_deformation.argtypes = [C.c_int] + [_f64p] * 4 + [_u8p, C.c_int64, C.c_int64, C.c_int] + [_f64p] * 5 + [_i32p]
        L.sid_grid_filter_device.argtypes = [vp] * 3 + flt + [vp] * 3
        L.sid_grid_deformation_device.argtypes = [vp] * 5 + [C.c_int64, C.c_int64, C.c_int] + [vp] * 7
        L.sid_grid_last_error.restype = C.c_char_p
        L.sid_grid_release.argtypes = [C.c_int]
    if hasattr(L, 'sid_grid_fill'):              # (absent from the libraries of earlier rounds that A/B runs load through SID_PM_LIB)
        vp, i64 = C.c_void_p, C.c_int64
        L.sid_grid_fill.argtypes = [C.c_int, _f64p, _f64p, _u8p, _u8p, i64, i64, C.c_int, C.c_int, C.c_int, _f64p, _f64p, _i32p]
        L.sid_grid_fill_device.argtypes = [vp] * 4 + [i64, i64, C.c_int, C.c_int, C.c_int] + [vp] * 4
        L.sid_grid_smooth.argtypes = [C.c_int, _f64p, _f64p, _u8p, i64, i64, _f64p, C.c_int, _f64p, _f64p]
        L.sid_grid_smooth_device.argtypes = [vp] * 3 + [i64, i64, _f64p, C.c_int] + [vp] * 3
    if hasattr(L, 'sid_warp_image'):
        vp = C.c_void_p
        tail = [C.c_int64, C.c_int64, vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_double,
                C.c_int, C.c_uint32, vp, C.c_int64, vp, vp, vp]
        L.sid_warp_image.argtypes = [C.c_int] + [_f64p] * 4 + [_u8p] + tail
        L.sid_warp_image_device.argtypes = [vp] * 5 + tail + [vp]
        L.sid_warp_last_error.restype = C.c_char_p
        L.sid_warp_release.argtypes = [C.c_int]
    if hasattr(L, 'sid_corr_lattice'):           # (absent from the libraries of earlier rounds that A/B runs load through SID_PM_LIB)
        vp, i64 = C.c_void_p, C.c_int64
        images = [vp, i64, vp, i64, i64, i64, C.c_int]
        L.sid_corr_lattice.argtypes = [C.c_int] + images + [i64] * 7 + [vp] * 3
        L.sid_corr_lattice_device.argtypes = images + [i64] * 7 + [vp] * 3 + [vp]
        L.sid_corr_points.argtypes = [C.c_int] + images + [vp] * 3 + [i64, i64] + [vp] * 3
        L.sid_corr_points_device.argtypes = images + [vp] * 3 + [i64, i64] + [vp] * 3 + [vp]
        L.sid_corr_last_error.restype = C.c_char_p
        L.sid_corr_release.argtypes = [C.c_int]
    if hasattr(L, 'sid_track_points'):           # (absent from the libraries of earlier rounds that A/B runs load through SID_PM_LIB)
        vp, i64 = C.c_void_p, C.c_int64
        L.sid_track_points.argtypes = [C.c_int] + [vp] * 5 + [i64, i64, C.c_int, C.c_uint32, vp, vp, i64, vp, vp, vp]
        L.sid_track_points_device.argtypes = [vp] * 5 + [i64, i64, C.c_int, C.c_uint32, vp, vp, i64, vp, vp, vp, vp]
        L.sid_track_last_error.restype = C.c_char_p
        L.sid_track_release.argtypes = [C.c_int]
    if hasattr(L, 'sid_ftg_knn2'):               # (absent from the libraries of earlier rounds that A/B runs load through SID_PM_LIB)
        vp, i64 = C.c_void_p, C.c_int64
        sets = [vp, vp, vp, i64, vp, vp, vp, i64, C.c_double]
        L.sid_ftg_knn2.argtypes = [C.c_int] + sets + [vp] * 3
        L.sid_ftg_knn2_device.argtypes = sets + [vp] * 5
        L.sid_ftg_workspace_bytes.argtypes = [i64, i64]
        L.sid_ftg_workspace_bytes.restype = i64
        L.sid_ftg_debug_plan.argtypes = [i64, i64] + [C.c_double] * 5 + [vp]
        L.sid_ftg_last_error.restype = C.c_char_p
        L.sid_ftg_release.argtypes = [C.c_int]
    if hasattr(L, 'sid_prep_apply'):
        vp, plane = C.c_void_p, [C.c_void_p, C.c_int64]
        L.sid_prep_subsample.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64] + plane + plane + [C.c_int, C.c_float, C.c_int64, vp, vp]
        L.sid_prep_apply.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64] + plane + plane + [C.c_int, C.c_float, _f64p] + plane + [vp]
        L.sid_prep_spatial_mean.argtypes = [C.c_int64, C.c_int64, _f64p, vp, C.c_int64, vp]
        L.sid_prep_debug_log10.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
        L.sid_prep_last_error.restype = C.c_char_p
    if hasattr(L, 'sid_mask_invalid'):
        vp, plane = C.c_void_p, [C.c_void_p, C.c_int64]
        raster = [vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp]          # d_wm, h, w, wm_stride, H, W, d_work
        L.sid_mask_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
        L.sid_mask_workspace_bytes.restype = C.c_int64
        L.sid_mask_landmask.argtypes = raster + plane + plane + [vp]
        L.sid_mask_invalid.argtypes = raster + plane + [C.c_int] + plane + [C.c_float] + plane + plane + [vp]
        L.sid_mask_last_error.restype = C.c_char_p
    if hasattr(L, 'sid_resize_f32'):
        vp, plane, i64 = C.c_void_p, [C.c_void_p, C.c_int64], C.c_int64
        L.sid_resize_f32.argtypes = [vp, i64, i64, i64, vp, i64, i64, i64, C.c_int, vp]
        L.sid_resize_u8.argtypes = [vp, i64, i64, i64, vp, i64, i64, i64, C.c_int, vp]
        L.sid_resize_prep_apply.argtypes = [vp, i64, i64, i64] + plane + plane + [C.c_int, C.c_float, _f64p, vp, i64, i64, i64, vp]
        L.sid_resize_prep_subsample.argtypes = [vp, i64, i64, i64] + plane + plane + [C.c_int, C.c_float, i64, i64, i64, vp, vp]
        L.sid_resize_last_error.restype = C.c_char_p
    # SID_PM_LIB (A/B runs against the library of an earlier round) may lack the entry points added since
    optional = ('sid_pm_check', 'sid_pm_unpermute', 'sid_pm_rotate_and_match', 'sid_pm_get_template', 'sid_pm_get_hessian', 'sid_pm_estimate_run_time') if os.environ.get('SID_PM_LIB') else ()
    for name in SYMBOLS:
        if name not in optional:
            getattr(L, name)                  # AttributeError here = header/library mismatch
    if L.sid_pm_abi_version() != ABI_VERSION and not os.environ.get('SID_PM_LIB'):
        raise ImportError('libsid_pm.so ABI %d != binding ABI %d' % (L.sid_pm_abi_version(), ABI_VERSION))
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        L = lib()
        msg = L.sid_pm_last_error() or L.sid_pm_strerror(rc)
        raise SidPmError(rc, msg.decode() if isinstance(msg, bytes) else str(msg))


def device_count():
    n = C.c_int(0)
    rc = lib().sid_pm_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def _u8(a):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise TypeError('images must be 2-D uint8 arrays (reference contract: lib.py:27-59)')
    if a.strides[1] != 1:
        a = np.ascontiguousarray(a)
    return a


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t):
    return a.ctypes.data_as(t)


def release_workspaces(device=-1):
    """Hand the cached device memory of the detector, the matcher, the first-guess evaluation and the deformation back
    (``sid_orb_release``, ``sid_ft_release``, ``sid_fg_release``, ``sid_defor_release``, ``sid_grid_release``, ``sid_warp_release``, ``sid_corr_release``, ``sid_track_release``, ``sid_ftg_release``; -1: every device).  No call on that device may be in flight.
    A process that never loaded the library has nothing cached: this returns without loading it (it is registered with
    atexit through pmlib.release_contexts, and loading means importing torch and initialising the GPU - not at interpreter
    shutdown, and not in a process that only used the host code)."""
    if _lib is None:
        return
    L = _lib
    for name in ('sid_orb_release', 'sid_ft_release', 'sid_fg_release', 'sid_defor_release', 'sid_grid_release', 'sid_warp_release',
                 'sid_corr_release', 'sid_track_release', 'sid_ftg_release'):
        if hasattr(L, name):
            getattr(L, name)(int(device))


def unpermute(stack_ptr, world, m, perm_ptr, n, out_ptr, ij_ptr, stream):
    """``sid_pm_unpermute`` on raw device(-visible) pointers (torch ``data_ptr()``) and a HIP stream handle."""
    _check(lib().sid_pm_unpermute(stack_ptr, int(world), int(m), perm_ptr, int(n), out_ptr, ij_ptr, stream))


def estimate_cost(border, img_size=34, n_angles=15, flags=HES_NORM):
    """Estimated nanoseconds per grid point (include/sid_pm.h sid_pm_estimate_cost): host arithmetic of the library.
    ``flags``: the flags of the run (they decide the Hessian's LDS layout, hence the class borders)."""
    b = _f64(border).ravel()
    out = np.empty(b.size, dtype=np.float64)
    _check(lib().sid_pm_estimate_cost(_p(b, _f64p), b.size, int(img_size), int(n_angles), int(flags), _p(out, _f64p)))
    return out


CLASS_PER_CU, CLASS_GS, CLASS_BIG, CLASS_LARGE = 15, 16, 32, 128          # include/sid_pm.h SID_PM_CLASS_*


def estimate_run_time(border, img_size=34, n_angles=15, flags=HES_NORM):
    """Estimated kernel time (ns) of one run over points with these borders (include/sid_pm.h sid_pm_estimate_run_time): point
    costs, launch tails, the launcher's side-by-side rule, large-window points - host arithmetic of the library."""
    b = _f64(border).ravel()
    t = C.c_double(0.0)
    _check(lib().sid_pm_estimate_run_time(_p(b, _f64p), b.size, int(img_size), int(n_angles), int(flags), C.byref(t)))
    return t.value


def estimate_residency(border, img_size=34, n_angles=15, flags=HES_NORM):
    """Launch class of each grid point (include/sid_pm.h sid_pm_estimate_residency): workgroups per CU (1 .. 4) in the low four
    bits (``& CLASS_PER_CU``), ``CLASS_GS`` for the launches that keep their per-placement sums in global memory, ``CLASS_BIG``
    for borders beyond 68 px; points of equal value share a launch."""
    b = _f64(border).ravel()
    out = np.empty(b.size, dtype=np.int32)
    _check(lib().sid_pm_estimate_residency(_p(b, _f64p), b.size, int(img_size), int(n_angles), int(flags), _p(out, _i32p)))
    return out


def rotation_terms(angle_deg, img_size):
    """(cos a, sin a, tcT0, tcT1) for one sampling angle, computed with NumPy exactly like the reference's get_template
    (pmlib.py:105-110): tc = int(s/2.)+1, a = radians(angle), transform = [[cos,-sin],[sin,cos]], tcT = [tc,tc].dot(transform).
    The C ABI requires these numbers from its caller (include/sid_pm.h: `rot`), so that the device samples the same float64
    coordinates the reference's scipy call would."""
    tc = int(img_size / 2.) + 1
    tc = np.array([tc, tc])
    a = np.radians(angle_deg)
    transform = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    tct = tc.dot(transform)
    return float(transform[0, 0]), float(transform[1, 0]), float(tct[0]), float(tct[1])


def rotation_table(angles, alpha0, img_size):
    """[K,4] table of rotation_terms(angle - alpha0) (pmlib.py:151)."""
    return np.array([rotation_terms(a - alpha0, img_size) for a in angles], dtype=np.float64).reshape(-1, 4)


def _rot_arg(rot, angles, alpha0, img_size):
    """The `rot` argument of the C ABI: the caller's table, or NumPy's own values (never the library's: sid_pm.h)."""
    rot = rotation_table(angles, alpha0, img_size) if rot is None else _f64(rot)
    if rot.shape != (len(angles), 4):
        raise ValueError('rot must be [n_angles, 4]')
    return rot


def rot_order_flag(order):
    """rot_order 0..5 as flag bits 3..5 (include/sid_pm.h SID_PM_ROT_ORDER); order 1 = ROT_ORDER1."""
    return (int(order) & 7) << 3


def flags_from_kwargs(hes_norm=True, hes_smth=False, mcc_norm=False, rot_order=0, subpixel=False):
    if isinstance(rot_order, bool) or rot_order not in (0, 1, 2, 3, 4, 5):
        raise ValueError('rot_order=%r: spline orders 0..5 (scipy.ndimage.affine_transform)' % (rot_order,))
    return ((HES_NORM if hes_norm else 0) | (HES_SMTH if hes_smth else 0) | (MCC_NORM if mcc_norm else 0) | rot_order_flag(rot_order)
            | (SUBPIXEL if subpixel else 0))


def pm_batch(img1, img2, c1, r1, c2fg, r2fg, border, img_size, alpha0, angles, rot=None, flags=HES_NORM):
    """One-shot host call == the Pool.map seam (pmlib.py:436-448).  -> (N,5) f64, (N,3) i32."""
    img1, img2 = _u8(img1), _u8(img2)
    v = [_f64(x) for x in (c1, r1, c2fg, r2fg, border)]
    n = len(v[0])
    angles = _f64(angles)
    rot = _rot_arg(rot, angles, alpha0, img_size) if len(angles) else _f64(np.zeros((0, 4)))
    rotp = _p(rot, _f64p)
    out = np.empty((n, 5), dtype=np.float64)
    ij = np.empty((n, 3), dtype=np.int32)
    _check(lib().sid_pm_batch(_p(img1, _u8p), img1.shape[0], img1.shape[1], img1.strides[0],
                              _p(img2, _u8p), img2.shape[0], img2.shape[1], img2.strides[0],
                              *[_p(x, _f64p) for x in v], n, int(img_size), float(alpha0),
                              _p(angles, _f64p), rotp, len(angles), int(flags), _p(out, _f64p), _p(ij, _i32p)))
    return out, ij


class PMContext(object):
    """Device-resident handle: images and points stay in HBM between runs."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(lib().sid_pm_create(int(device), C.byref(self._h)))
        self.device = int(device)
        self.n = 0
        self._keep = []
        # (rows, cols) of image 2 per owned slot and of the borrowed binding, and which of them is current - the C handle's
        # cur / cur_slot mirrored, for rotate_and_match(window=None)
        self._shape2 = {}
        self._cur = None

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            lib().sid_pm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except TypeError:                                  # interpreter shutdown: the module globals are already gone
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream_handle):
        _check(lib().sid_pm_set_stream(self._h, C.c_void_p(int(stream_handle) if stream_handle else 0)))

    def upload_pair(self, img1, img2, slot=0, select=True):
        """Copy a host pair into device slot 0/1 and (select=True) make it the pair the next run matches.
        Streaming code that prefetches pair k+1 while pair k runs passes select=False and switches with
        select_pair (the C call alone only selects a slot when no other owned slot is current)."""
        img1, img2 = _u8(img1), _u8(img2)
        self._keep = (self._keep + [img1, img2])[-4:]  # async copies: keep the host buffers of both slots alive
        _check(lib().sid_pm_upload_pair(self._h, int(slot),
                                        _p(img1, _u8p), img1.shape[0], img1.shape[1], img1.strides[0],
                                        _p(img2, _u8p), img2.shape[0], img2.shape[1], img2.strides[0]))
        self._uploaded(slot, img2)
        if select:
            self.select_pair(slot)

    def _uploaded(self, slot, img2):
        """Image 2 of ``slot`` has this shape now; the slot becomes current as in sid_pm_upload_pair: the first pair, a refresh
        of the selected slot, or a borrowed binding was current."""
        self._shape2[int(slot)] = (int(img2.shape[0]), int(img2.shape[1]))
        if self._cur is None or self._cur == int(slot) or self._cur == 'bound':
            self._cur = int(slot)

    def upload_pair_background(self, img1, img2, slot=0):
        """upload_pair on a worker thread, entered before this returns: the C call runs without the interpreter lock,
        so host work of the caller (however long it keeps the lock itself) overlaps the copy.  Returns an object
        whose wait() joins the thread and re-raises what the upload raised."""
        import threading
        img1, img2 = _u8(img1), _u8(img2)
        self._keep = (self._keep + [img1, img2])[-4:]
        fn, h, s = lib().sid_pm_upload_pair, self._h, int(slot)
        args = (h, s, _p(img1, _u8p), img1.shape[0], img1.shape[1], img1.strides[0],
                _p(img2, _u8p), img2.shape[0], img2.shape[1], img2.strides[0])
        box = {'rc': None, 'exc': None, 'msg': None}
        entered = threading.Event()
        last_error = lib().sid_pm_last_error

        def run():
            try:
                entered.set()                       # the next thing this thread does is the C call (lock released there)
                box['rc'] = fn(*args)
                if box['rc'] != 0:                  # the library's error text is thread-local: read it on this thread
                    box['msg'] = last_error()
            except BaseException as e:              # noqa: handed to the waiting thread
                box['exc'] = e

        t = threading.Thread(target=run, daemon=True)
        t.start()
        entered.wait()
        self._uploaded(s, img2)
        ctx = self

        class _Pending:
            def wait(self_inner):
                t.join()
                if box['exc'] is not None:
                    raise box['exc']
                if box['rc'] != 0:
                    msg = box['msg'] or lib().sid_pm_strerror(box['rc'])
                    raise SidPmError(box['rc'], msg.decode() if isinstance(msg, bytes) else str(msg))
                ctx.select_pair(s)
        return _Pending()

    def select_pair(self, slot):
        _check(lib().sid_pm_select_pair(self._h, int(slot)))
        self._cur = int(slot)

    def bind_pair_ptr(self, p1, rows1, cols1, stride1, p2, rows2, cols2, stride2):
        _check(lib().sid_pm_bind_pair(self._h, C.c_void_p(int(p1)), rows1, cols1, stride1,
                                      C.c_void_p(int(p2)), rows2, cols2, stride2))
        self._shape2['bound'] = (int(rows2), int(cols2))
        self._cur = 'bound'

    def bind_pair_tensors(self, t1, t2):
        """Borrow two CUDA/HIP uint8 torch tensors (2-D, unit inner stride); they stay borrowed until the next bind / upload /
        select.  When their pixels are read: with rot_order 0 and 1 at every ``run()``, so tensors overwritten in place (on the
        handle's stream, or synchronised) are matched with their new content.  With rot_order 2..5 the spline coefficients of
        image 1 and the templates of the resident points sampled from them are computed at the first ``run()`` after the bind and
        kept: after changing the pixels in place call ``bind_pair_tensors`` again - with the same tensors - or the next run
        matches the templates of the old image 1 (include/sid_pm.h sid_pm_bind_pair)."""
        for t in (t1, t2):
            if t.dim() != 2 or t.stride(1) != 1 or str(t.dtype) != 'torch.uint8' or not t.is_cuda:
                raise TypeError('need 2-D uint8 device tensors with unit inner stride')
        self._keep = [t1, t2]
        self.bind_pair_ptr(t1.data_ptr(), t1.shape[0], t1.shape[1], t1.stride(0),
                           t2.data_ptr(), t2.shape[0], t2.shape[1], t2.stride(0))

    def set_points(self, c1, r1, c2fg, r2fg, border, img_size, alpha0, angles, rot=None, flags=HES_NORM):
        v = [_f64(x) for x in (c1, r1, c2fg, r2fg, border)]
        n = len(v[0])
        if any(len(x) != n for x in v):
            raise ValueError('point vectors differ in length')
        angles = _f64(angles)
        rot = _rot_arg(rot, angles, alpha0, img_size) if len(angles) else _f64(np.zeros((0, 4)))
        rotp = _p(rot, _f64p)
        _check(lib().sid_pm_set_points(self._h, *[_p(x, _f64p) for x in v], n, int(img_size), float(alpha0),
                                       _p(angles, _f64p), rotp, len(angles), int(flags)))
        self.n = n

    def bind_results_tensors(self, t_out, t_ij=None):
        """Write results into caller-owned device tensors: float64 [n,5] and int32 [n,3]."""
        if tuple(t_out.shape) != (self.n, 5) or str(t_out.dtype) != 'torch.float64' or not t_out.is_contiguous():
            raise TypeError('t_out must be a contiguous float64 [n,5] device tensor')
        if t_ij is not None and (tuple(t_ij.shape) != (self.n, 3) or str(t_ij.dtype) != 'torch.int32'
                                 or not t_ij.is_contiguous()):
            raise TypeError('t_ij must be a contiguous int32 [n,3] device tensor')
        self._keep_out = (t_out, t_ij)
        _check(lib().sid_pm_bind_results(self._h, C.c_void_p(t_out.data_ptr()),
                                         C.c_void_p(t_ij.data_ptr()) if t_ij is not None else None))

    def bind_results_host(self):
        """Zero-copy results: allocate pinned host tensors float64 [n,5] / int32 [n,3] and make the kernels write their 52 B per
        point straight into them (pinned memory is device-visible on ROCm).  After ``run()`` + ``sync()`` the tensors hold
        the results - no copy after the kernels, which is worth 1 % of a 40 000-point step and more of a shorter one.
        Returns (out, ij); they stay bound until the next ``set_points`` / ``bind_results_tensors``."""
        import torch
        out = torch.empty((self.n, 5), dtype=torch.float64, pin_memory=True)
        ij = torch.empty((self.n, 3), dtype=torch.int32, pin_memory=True)
        self.bind_results_tensors(out, ij)
        return out, ij

    def run(self):
        _check(lib().sid_pm_run(self._h))

    def sync(self):
        _check(lib().sid_pm_sync(self._h))

    def check(self):
        """Raise if a launch refused a point with a valid window (``sid_pm_check``); for callers that synchronise the
        stream themselves (torch) instead of through ``sync`` / ``fetch``."""
        if hasattr(lib(), 'sid_pm_check'):
            _check(lib().sid_pm_check(self._h))

    def fetch(self, want_ij=True):
        out = np.empty((self.n, 5), dtype=np.float64)
        ij = np.empty((self.n, 3), dtype=np.int32) if want_ij else None
        _check(lib().sid_pm_fetch(self._h, _p(out, _f64p), _p(ij, _i32p) if want_ij else None))
        return (out, ij) if want_ij else out

    def device_results(self):
        a, b = C.c_void_p(), C.c_void_p()
        _check(lib().sid_pm_device_results(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def work_info(self):
        info = np.zeros(6, dtype=np.float64)
        _check(lib().sid_pm_work_info(self._h, _p(info, _f64p)))
        return dict(launches=int(info[0]), valid_points=int(info[1]), macs=float(info[2]),
                    hbm_bytes=float(info[3]), max_lds_bytes=int(info[4]))

    def debug_point(self, c1, r1, c2fg, r2fg, border, img_size, alpha0, angles, rot=None, flags=HES_NORM,
                    cap=256 * 256):
        angles = _f64(angles)
        rot = _rot_arg(rot, angles, alpha0, img_size)
        rotp = _p(rot, _f64p)
        K, s = len(angles), int(img_size)
        tm = np.zeros((K, s, s), dtype=np.uint8)
        ccm = np.zeros(cap, dtype=np.float32)
        hes = np.zeros(cap, dtype=np.float32)
        shape = np.zeros(2, dtype=np.int32)
        out5 = np.zeros(5, dtype=np.float64)
        ij3 = np.zeros(3, dtype=np.int32)
        cyc = np.zeros(32, dtype=np.int64)
        _check(lib().sid_pm_debug_point(self._h, float(c1), float(r1), float(c2fg), float(r2fg), float(border), s,
                                        float(alpha0), _p(angles, _f64p), rotp, K, int(flags), _p(tm, _u8p),
                                        _p(ccm, _f32p), _p(hes, _f32p), cap, _p(shape, _i32p), _p(out5, _f64p),
                                        _p(ij3, _i32p), cyc.ctypes.data_as(C.POINTER(C.c_int64))))
        rh, rw = int(shape[0]), int(shape[1])
        n = rh * rw
        return dict(templates=tm, ccm=ccm[:n].reshape(rh, rw), hes=hes[:n].reshape(rh, rw), out=out5, ij=ij3,
                    cycles=cyc)

    def rotate_and_match(self, c1, r1, img_size, alpha0, angles, rot=None, flags=HES_NORM, window=None, want_ccm=True,
                         want_template=True):
        """``sid_pm_rotate_and_match`` on the handle's current pair: the templates around (c1, r1) of image 1 against ``window`` =
        (row0, col0, rows, cols) of image 2 (None: the whole of image 2 of the current pair).  -> dict(out = dc, dr, a, r, h; ij = peak row, peak column,
        angle index (-1: NaN point); ccm [rh, rw] float32 and template [s, s] uint8, None for a NaN point)."""
        angles = _f64(angles)
        rot = _rot_arg(rot, angles, alpha0, img_size)
        s = int(img_size)
        if window is None:
            if self._cur is None:
                raise ValueError('rotate_and_match needs an image pair (upload_pair / bind_pair first)')
            window = (0, 0) + self._shape2[self._cur]
        r0, c0, wh, ww = [int(v) for v in window]
        rh, rw = wh - s + 1, ww - s + 1
        out5 = np.zeros(5, dtype=np.float64)
        ij3 = np.zeros(3, dtype=np.int32)
        ccm = np.zeros(max(rh, 0) * max(rw, 0), dtype=np.float32) if want_ccm else None
        tm = np.zeros((s, s), dtype=np.uint8) if want_template else None
        _check(lib().sid_pm_rotate_and_match(self._h, float(c1), float(r1), s, r0, c0, wh, ww, float(alpha0), _p(angles, _f64p),
                                             _p(rot, _f64p), len(angles), int(flags), _p(out5, _f64p), _p(ij3, _i32p),
                                             _p(ccm, _f32p) if want_ccm else None, ccm.size if want_ccm else 0,
                                             _p(tm, _u8p) if want_template else None))
        ok = ij3[2] >= 0
        return dict(out=out5, ij=ij3, ccm=ccm.reshape(rh, rw) if (want_ccm and ok) else None,
                    template=tm if (want_template and ok) else None)

    def debug_rsqrt(self, x):
        x = _f64(x)
        y = np.empty_like(x)
        _check(lib().sid_pm_debug_rsqrt(self._h, _p(x, _f64p), _p(y, _f64p), x.size))
        return y

    def debug_ncc_selftest(self, evaluations, img_size=34, seed=1):
        """(evaluations, mismatches, spec-route evaluations) of the shortened NCC normalisation against the full one."""
        counts = (C.c_uint64 * 3)()
        _check(lib().sid_pm_debug_ncc_selftest(self._h, int(seed), int(evaluations), int(img_size), counts))
        return int(counts[0]), int(counts[1]), int(counts[2])

    def debug_hypot_selftest(self, evaluations, seed=1):
        """(evaluations, mismatches) of the kernel's shortened hypotf against the IEEE route, on the device."""
        counts = (C.c_uint64 * 2)()
        _check(lib().sid_pm_debug_hypot_selftest(self._h, int(seed), int(evaluations), counts))
        return int(counts[0]), int(counts[1])


def get_template(img, c, r, rot4, img_size, rot_order=0, device=0):
    """``sid_pm_get_template``: the s x s uint8 template around (c, r) of a host uint8 image (pmlib.py:89-115), ``rot_order``
    0..5; ``rot4`` = (cos a, sin a, tcT0, tcT1), every entry finite and below 1e6 in magnitude (SidPmError -1 otherwise)."""
    img = _u8(img)
    rot4 = _f64(rot4).reshape(4)
    s = int(img_size)
    out = np.empty((s, s), dtype=np.uint8)
    _check(lib().sid_pm_get_template(int(device), _p(img, _u8p), img.shape[0], img.shape[1], img.strides[0], float(c), float(r),
                                     _p(rot4, _f64p), s, int(rot_order), _p(out, _u8p)))
    return out


def get_hessian(ccm, flags=HES_NORM, device=0):
    """``sid_pm_get_hessian``: the Hessian magnitudes of a float32 matrix (pmlib.py:36-59)."""
    ccm = np.ascontiguousarray(ccm, dtype=np.float32)
    if ccm.ndim != 2:
        raise ValueError('get_hessian needs a 2-D matrix')
    out = np.empty_like(ccm)
    _check(lib().sid_pm_get_hessian(int(device), _p(ccm, _f32p), ccm.shape[0], ccm.shape[1], int(flags), _p(out, _f32p)))
    return out


def _checker(unit, index_error=None):
    """The return-code check of one unit of the library: raises SidPmError with the unit's own ``<unit>_last_error`` text
    (IndexError for the code ``index_error``)."""
    def check(rc):
        if rc != 0:
            msg = getattr(lib(), unit + '_last_error')().decode()
            raise IndexError(msg) if rc == index_error else SidPmError(rc, msg)
    return check


_ft_check, _stage_check, _fg_check = _checker('sid_ft'), _checker('sid_stage'), _checker('sid_fg')
_defor_check, _grid_check, _warp_check = _checker('sid_defor', DEFOR_ERR_INDEX), _checker('sid_grid'), _checker('sid_warp')
_prep_check, _mask_check, _resize_check = _checker('sid_prep'), _checker('sid_mask'), _checker('sid_resize')
_corr_check, _track_check, _ftg_check = _checker('sid_corr'), _checker('sid_track'), _checker('sid_ftg')


def _vp(p):
    """An optional pointer argument: a raw address (0 or None: null) or a NumPy array (None: null)."""
    if isinstance(p, np.ndarray):
        p = p.ctypes.data
    return C.c_void_p(int(p)) if p else None


def ft_knn2(desc1, desc2, device=0):
    """Two nearest train descriptors (Hamming) of every query descriptor: include/sid_ft.h sid_ft_knn2.

    desc1 [n1,32], desc2 [n2,32] uint8 -> (idx [n1,2] int32, dist [n1,2] int32), -1 where absent."""
    d1 = np.ascontiguousarray(desc1, dtype=np.uint8).reshape(-1, 32)
    d2 = np.ascontiguousarray(desc2, dtype=np.uint8).reshape(-1, 32)
    idx = np.empty((len(d1), 2), dtype=np.int32)
    dist = np.empty((len(d1), 2), dtype=np.int32)
    L = lib()
    _ft_check(L.sid_ft_knn2(int(device), d1.ctypes.data_as(_u8p), len(d1), d2.ctypes.data_as(_u8p), len(d2),
                            idx.ctypes.data_as(_i32p), dist.ctypes.data_as(_i32p)))
    return idx, dist


class _FtPlan(C.Structure):
    """struct sid_ft_plan (include/sid_ft.h)."""
    _fields_ = [(name, C.c_int64) for name in ('mfma', 'chunk', 'nchunks', 'n1pad', 'n2pad')]


def ft_debug_plan(n1, n2):
    """The plan sid_ft_knn2_device follows for n1 x n2 descriptors (include/sid_ft.h sid_ft_debug_plan; test support, no
    device call): a dict of the struct's fields."""
    s = _FtPlan()
    _ft_check(lib().sid_ft_debug_plan(int(n1), int(n2), C.byref(s)))
    return {name: int(getattr(s, name)) for name, _ in _FtPlan._fields_}


def ft_workspace_bytes(n1, n2):
    """Bytes of workspace ft_knn2_device needs for n1 x n2 descriptors (include/sid_ft.h sid_ft_workspace_bytes)."""
    return int(lib().sid_ft_workspace_bytes(int(n1), int(n2)))


def ft_knn2_device(d_desc1, n1, d_desc2, n2, d_idx, d_dist, d_workspace, stream=0):
    """ft_knn2 on device-resident buffers, asynchronous on ``stream`` (include/sid_ft.h sid_ft_knn2_device): raw device
    addresses of desc1 [n1,32] and desc2 [n2,32] uint8 (16-byte aligned), idx and dist [n1,2] int32, and a workspace of
    ft_workspace_bytes(n1, n2) bytes (16-byte aligned)."""
    _ft_check(lib().sid_ft_knn2_device(_vp(d_desc1), int(n1), _vp(d_desc2), int(n2), _vp(d_idx), _vp(d_dist), _vp(d_workspace),
                                       _vp(stream)))


def _ftg_radius(radius):
    """The radius of the guided matcher as a float: finite and >= 0, or ValueError (before any device call)."""
    r = float(radius)
    if not (np.isfinite(r) and r >= 0.0):
        raise ValueError('search radius must be finite and >= 0, got %r' % (radius,))
    return r


def _ftg_set(desc, xy, what):
    """One side of the guided matcher: descriptors uint8 [n, 32] and positions [n, 2] -> (desc, x, y) C-contiguous."""
    d = np.asarray(desc)
    if d.dtype != np.uint8 or d.ndim != 2 or d.shape[1] != 32:
        raise TypeError('%s descriptors must be a uint8 array of shape (n, 32)' % what)
    p = np.asarray(xy, dtype=np.float64)
    if p.ndim != 2 or p.shape != (len(d), 2):
        raise ValueError('%s positions must have shape (%d, 2): one (x, y) per descriptor, got %r' % (what, len(d), p.shape))
    return np.ascontiguousarray(d), np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])


def ftg_knn2(desc1, q_xy, desc2, t_xy, radius, device=0, want_count=True):
    """Two Hamming-nearest train descriptors of every query among those within ``radius`` pixels of the query's position:
    include/sid_ftg.h sid_ftg_knn2.

    desc1 [n1,32], desc2 [n2,32] uint8; q_xy [n1,2]: the PREDICTED positions of the queries in the train image's pixel frame,
    t_xy [n2,2]: the train positions -> (idx [n1,2] int32, dist [n1,2] int32, count [n1] int32 or None), -1 where absent.
    Shapes, dtypes and the radius are checked before any device call (TypeError / ValueError)."""
    d1, qx, qy = _ftg_set(desc1, q_xy, 'query')
    d2, tx, ty = _ftg_set(desc2, t_xy, 'train')
    r = _ftg_radius(radius)
    if len(d2) >= FTG_MAX_TRAIN:
        raise ValueError('at most %d train descriptors' % (FTG_MAX_TRAIN - 1))
    n1 = len(d1)
    idx = np.empty((n1, 2), dtype=np.int32)
    dist = np.empty((n1, 2), dtype=np.int32)
    count = np.empty(n1, dtype=np.int32) if want_count else None
    if n1:                                                               # (an empty array has no address to hand over)
        _ftg_check(lib().sid_ftg_knn2(int(device), _vp(d1), _vp(qx), _vp(qy), n1, _vp(d2), _vp(tx), _vp(ty), len(d2), r,
                                      _vp(idx), _vp(dist), _vp(count)))
    return idx, dist, count


def ftg_workspace_bytes(n1, n2):
    """Bytes of workspace ftg_knn2_device needs (include/sid_ftg.h sid_ftg_workspace_bytes)."""
    return int(lib().sid_ftg_workspace_bytes(int(n1), int(n2)))


def ftg_knn2_device(d_desc1, d_qx, d_qy, n1, d_desc2, d_tx, d_ty, n2, radius, d_idx, d_dist, d_count, d_workspace, stream=0):
    """ftg_knn2 on device-resident buffers, asynchronous on ``stream`` (include/sid_ftg.h sid_ftg_knn2_device): raw device
    addresses (torch ``data_ptr()``; d_count 0 for none) of descriptors [n,32] uint8 (16-byte aligned), positions [n] float64,
    idx and dist [n1,2] int32, count [n1] int32 and a workspace of ftg_workspace_bytes(n1, n2) bytes (16-byte aligned)."""
    r = _ftg_radius(radius)
    _ftg_check(lib().sid_ftg_knn2_device(_vp(d_desc1), _vp(d_qx), _vp(d_qy), int(n1), _vp(d_desc2), _vp(d_tx), _vp(d_ty), int(n2), r,
                                         _vp(d_idx), _vp(d_dist), _vp(d_count), _vp(d_workspace), _vp(stream)))


class _FtgPlan(C.Structure):
    """struct sid_ftg_plan (include/sid_ftg.h)."""
    _fields_ = [(name, C.c_double) for name in ('x0', 'y0', 'cell_x', 'cell_y')] + \
               [(name, C.c_int64) for name in ('nx', 'ny', 'axis_cap', 'max_items', 'workspace_bytes')]


def ftg_debug_plan(n1, n2, box, radius):
    """What csrc/ft_guided_plan.h computes for n1 queries, n2 train points with the bounding box ``box`` = (x_lo, x_hi, y_lo,
    y_hi) and ``radius`` (include/sid_ftg.h sid_ftg_debug_plan; test support, no device call): a dict of the struct's fields."""
    s = _FtgPlan()
    _ftg_check(lib().sid_ftg_debug_plan(int(n1), int(n2), *[float(v) for v in box], float(radius), C.byref(s)))
    return {name: getattr(s, name) for name, _ in _FtgPlan._fields_}


class _FgRoute(C.Structure):
    """struct sid_fg_route (include/sid_fg.h)."""
    _fields_ = [(name, C.c_int64) for name in ('buckets', 'entries', 'capacity', 'ychunks', 'chunk')]


def fg_debug_route():
    """Which route the calling thread's last first-guess call took (include/sid_fg.h sid_fg_debug_route; test support): a
    dict of the struct's fields."""
    s = _FgRoute()
    _fg_check(lib().sid_fg_debug_route(C.byref(s)))
    return {name: int(getattr(s, name)) for name, _ in _FgRoute._fields_}


class _StageRoute(C.Structure):
    """struct sid_stage_route (include/sid_stage.h)."""
    _fields_ = [('n_valid', C.c_int64), ('below', C.c_int64 * 4), ('inside', C.c_int64 * 4),
                ('lo', C.c_uint32 * 4), ('span', C.c_uint32 * 4), ('shift', C.c_uint32 * 4),
                ('m_valid', C.c_uint32), ('n_hint', C.c_int32),
                ('n_direct', C.c_int32), ('n_resolved', C.c_int32), ('n_radix', C.c_int32),
                ('resolve_passes', C.c_int32), ('resolve_states', C.c_int32), ('image_passes', C.c_int32)]


class StageWorkspace(object):
    """Persistent device + pinned host buffers of the staging step (include/sid_stage.h sid_stage_create)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _stage_check(lib().sid_stage_create(int(device), C.byref(self._h)))

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            lib().sid_stage_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except TypeError:                                  # interpreter shutdown: the module globals are already gone
            pass

    def begin(self, ptr, rows, cols, stride, stream=0, fractions=None):
        """First pass: number of non-NaN pixels; keeps what order_stats needs - the leading-digit histogram, or (``fractions``:
        where the wanted order statistics lie, as fractions of the non-NaN pixels) the histograms inside sampled key ranges
        around them, which saves order_stats one of its two passes (include/sid_stage.h sid_stage_begin_hint)."""
        n = C.c_int64(0)
        if fractions is not None and len(fractions) > 0:
            f = np.ascontiguousarray(fractions, dtype=np.float64)
            _stage_check(lib().sid_stage_begin_hint(self._h, _vp(ptr), rows, cols, stride,
                                                    f.ctypes.data_as(C.POINTER(C.c_double)), len(f), C.byref(n), _vp(stream)))
        else:
            _stage_check(lib().sid_stage_begin(self._h, _vp(ptr), rows, cols, stride, C.byref(n), _vp(stream)))
        return int(n.value)

    def order_stats(self, ranks):
        r = np.ascontiguousarray(ranks, dtype=np.int64)
        out = np.empty(len(r), dtype=np.float32)
        _stage_check(lib().sid_stage_order_stats_ws(self._h, r.ctypes.data_as(C.POINTER(C.c_int64)), len(r), out.ctypes.data_as(_f32p)))
        return out

    def route(self):
        """Which route the last begin / order_stats took (include/sid_stage.h sid_stage_debug_route; test support): a dict of
        the struct's fields, the per-range ones as lists of n_hint Python ints."""
        s = _StageRoute()
        _stage_check(lib().sid_stage_debug_route(self._h, C.byref(s)))
        d = {name: int(getattr(s, name)) for name, kind in _StageRoute._fields_ if not hasattr(kind, '_length_')}
        for name in ('lo', 'span', 'shift', 'below', 'inside'):
            d[name] = [int(v) for v in getattr(s, name)[:d['n_hint']]]
        return d


def stage_count_valid(ptr, rows, cols, stride, stream=0):
    """Non-NaN pixels of a device float32 image (include/sid_stage.h)."""
    n = C.c_int64(0)
    _stage_check(lib().sid_stage_count_valid(_vp(ptr), rows, cols, stride, C.byref(n), _vp(stream)))
    return int(n.value)


def stage_order_stats(ptr, rows, cols, stride, ranks, stream=0):
    """Exact order statistics (0-based ranks among the non-NaN pixels) of a device float32 image."""
    r = np.ascontiguousarray(ranks, dtype=np.int64)
    out = np.empty(len(r), dtype=np.float32)
    _stage_check(lib().sid_stage_order_stats(_vp(ptr), rows, cols, stride, r.ctypes.data_as(C.POINTER(C.c_int64)),
                                             len(r), out.ctypes.data_as(_f32p), _vp(stream)))
    return out


def stage_scale_u8(ptr, rows, cols, stride, vmin, denom, out_ptr, out_stride, stream=0):
    _stage_check(lib().sid_stage_scale_u8(_vp(ptr), rows, cols, stride, float(vmin), float(denom),
                                          _vp(out_ptr), out_stride, _vp(stream)))


def fg_interp_linear(pts, simplices, values, q, device=0, details=False):
    """Piecewise-linear interpolation of two value columns at the points q in a given triangulation
    (include/sid_fg.h sid_fg_interp_linear): pts [n,2], simplices [m,3], values [n,2], q [k,2] -> [k,2] (NaN outside).
    details=True: also the simplex index per query (-1: none) and the doubt flags (queries on an edge, a vertex, the hull,
    or with a value next to a half-integer: to be evaluated with SciPy by the caller)."""
    pts, values, q = _f64(pts), _f64(values), _f64(q)
    simp = np.ascontiguousarray(simplices, dtype=np.int32)
    out = np.empty((len(q), 2), dtype=np.float64)
    sx = np.empty(len(q), dtype=np.int32)
    dbt = np.empty(len(q), dtype=np.int32)
    L = lib()
    _fg_check(L.sid_fg_interp_linear(int(device), _p(pts, _f64p), len(pts), simp.ctypes.data_as(_i32p), len(simp), _p(values, _f64p),
                                     _p(q, _f64p), len(q), _p(out, _f64p), sx.ctypes.data_as(_i32p), dbt.ctypes.data_as(_i32p)))
    return (out, sx, dbt.astype(bool)) if details else out


def fg_nearest_dist(seeds, q, device=0):
    """Distance from every point of q [k,2] to the nearest of seeds [n,2] (include/sid_fg.h sid_fg_nearest_dist)."""
    seeds, q = _f64(seeds), _f64(q)
    out = np.empty(len(q), dtype=np.float64)
    L = lib()
    _fg_check(L.sid_fg_nearest_dist(int(device), _p(seeds, _f64p), len(seeds), _p(q, _f64p), len(q), _p(out, _f64p)))
    return out


def fg_distance_image(seeds, rows, cols, device=0):
    """Distance of every pixel of a rows x cols image to the nearest of seeds [n,2] = (row, column)
    (include/sid_fg.h sid_fg_distance_image) -> float64 [rows, cols]."""
    seeds = _f64(seeds)
    out = np.empty((int(rows), int(cols)), dtype=np.float64)
    L = lib()
    _fg_check(L.sid_fg_distance_image(int(device), _p(seeds, _f64p), len(seeds), int(rows), int(cols), _p(out, _f64p)))
    return out


def fg_knn(seeds, values, q, k=5, max_dist=None, device=0, details=False):
    """Component-wise median of values [n,2] over the k nearest of seeds [n,2] at every point of q [m,2] -> [m,2]
    (include/sid_fg.h sid_fg_knn; not the reference's method).  ``max_dist``: seeds further away do not count (None: no
    limit); a query without a neighbour gives NaN.  Seeds with a non-finite coordinate or value never take part.
    ``device=-1``: the kernels' source in a host loop (tests, machines without a GPU).  details=True: also the number of
    neighbours per query, int32 [m], and their seed indices in ascending (distance, index) order, int32 [m,k] padded with -1."""
    seeds, values, q = _f64(seeds).reshape(-1, 2), _f64(values).reshape(-1, 2), _f64(q).reshape(-1, 2)
    if len(values) != len(seeds):
        raise ValueError('seeds and values differ in length')
    k = int(k)
    out = np.empty((len(q), 2), dtype=np.float64)
    cnt = np.empty(len(q), dtype=np.int32)
    idx = np.empty((len(q), min(max(k, 0), 16)), dtype=np.int32)
    L = lib()
    _fg_check(L.sid_fg_knn(int(device), _p(seeds, _f64p), len(seeds), _p(values, _f64p), _p(q, _f64p), len(q), k,
                           float('inf') if max_dist is None else float(max_dist), _p(out, _f64p),
                           _p(cnt, _i32p) if details else None, _p(idx, _i32p) if details else None))
    return (out, cnt, idx) if details else out


def defor_triangulation(x, y, u, v, t, device=0):
    """``sid_defor_triangulation`` on host arrays: x, y, u, v float64 [n], t int32 / int64 [m, 3] (C-contiguous)
    -> e1, e2, e3, a, p float64 [m].  An index outside [-n, n) raises IndexError."""
    m = len(t)
    out = [np.empty(m, dtype=np.float64) for _ in range(5)]
    _defor_check(lib().sid_defor_triangulation(int(device), *[_p(a, _f64p) for a in (x, y, u, v)], len(x),
                                               _vp(t), int(t.dtype == np.int64), m,
                                               *[_p(a, _f64p) for a in out]))
    return tuple(out)


def defor_elems(x, y, u, v, a, device=0):
    """``sid_defor_elems`` on host arrays: x, y, u, v float64 [3, m], a float64 [m] (C-contiguous) -> e1, e2, e3 float64 [m]."""
    m = len(a)
    out = [np.empty(m, dtype=np.float64) for _ in range(3)]
    _defor_check(lib().sid_defor_elems(int(device), *[_p(b, _f64p) for b in (x, y, u, v, a)], m, *[_p(b, _f64p) for b in out]))
    return tuple(out)


def defor_triangulation_device(x, y, u, v, n, t, t_int64, m, outs, stream):
    """``sid_defor_triangulation_device`` on raw device pointers (torch ``data_ptr()``): outs = (e1, e2, e3, a, p)."""
    _defor_check(lib().sid_defor_triangulation_device(*[_vp(q) for q in (x, y, u, v)], int(n), _vp(t),
                                                      int(bool(t_int64)), int(m), *[_vp(q) for q in outs],
                                                      _vp(stream)))


def defor_elems_device(x, y, u, v, a, m, outs, stream):
    """``sid_defor_elems_device`` on raw device pointers: x, y, u, v [3, m], a [m]; outs = (e1, e2, e3)."""
    _defor_check(lib().sid_defor_elems_device(*[_vp(q) for q in (x, y, u, v, a)], int(m),
                                              *[_vp(q) for q in outs], _vp(stream)))


def defor_debug_hypot(x, y, device=0):
    """hypot(x, y) elementwise as the deformation kernel evaluates it (``sid_defor_debug_hypot``): on HIP device ``device``,
    or with the same source compiled for the host (device=-1)."""
    x, y = _f64(x).ravel(), _f64(y).ravel()
    if x.size != y.size:
        raise ValueError('x and y differ in size')
    out = np.empty_like(x)
    _defor_check(lib().sid_defor_debug_hypot(int(device), _p(x, _f64p), _p(y, _f64p), x.size, _p(out, _f64p)))
    return out


def _opt_u8(valid):
    return _p(valid, _u8p) if valid is not None else None


def grid_filter(u, v, valid, eps, threshold, radius, min_neighbours, device=0):
    """``sid_grid_filter`` on host arrays: u, v float64 [rows, cols], valid uint8 [rows, cols] or None (C-contiguous)
    -> keep uint8 [rows, cols], res float64 [rows, cols].  device=-1: the kernels' source in a host loop (tests)."""
    rows, cols = u.shape
    keep, res = np.empty((rows, cols), dtype=np.uint8), np.empty((rows, cols), dtype=np.float64)
    _grid_check(lib().sid_grid_filter(int(device), _p(u, _f64p), _p(v, _f64p), _opt_u8(valid), rows, cols, float(eps),
                                      float(threshold), int(radius), int(min_neighbours), _p(keep, _u8p), _p(res, _f64p)))
    return keep, res


def grid_deformation(x, y, u, v, valid, diagonal, device=0):
    """``sid_grid_deformation`` on host arrays: x, y, u, v float64 [rows, cols] (rows, cols >= 2), valid uint8 or None,
    diagonal a SID_GRID_DIAG_* code -> e1, e2, e3, a, p float64 [rows-1, cols-1, 2], t int32 [rows-1, cols-1, 2, 3]."""
    rows, cols = x.shape
    out = [np.empty((rows - 1, cols - 1, 2), dtype=np.float64) for _ in range(5)]
    t = np.empty((rows - 1, cols - 1, 2, 3), dtype=np.int32)
    _grid_check(lib().sid_grid_deformation(int(device), *[_p(a, _f64p) for a in (x, y, u, v)], _opt_u8(valid), rows, cols,
                                           int(diagonal), *[_p(a, _f64p) for a in out], _p(t, _i32p)))
    return tuple(out) + (t,)


def grid_filter_device(u, v, valid, rows, cols, eps, threshold, radius, min_neighbours, keep, res, stream):
    """``sid_grid_filter_device`` on raw device pointers (torch ``data_ptr()``; valid 0 for none)."""
    _grid_check(lib().sid_grid_filter_device(*[_vp(q) for q in (u, v, valid)], int(rows), int(cols), float(eps),
                                             float(threshold), int(radius), int(min_neighbours), _vp(keep),
                                             _vp(res), _vp(stream)))


def grid_deformation_device(x, y, u, v, valid, rows, cols, diagonal, outs, stream):
    """``sid_grid_deformation_device`` on raw device pointers: outs = (e1, e2, e3, a, p, t)."""
    _grid_check(lib().sid_grid_deformation_device(*[_vp(q) for q in (x, y, u, v, valid)], int(rows), int(cols),
                                                  int(diagonal), *[_vp(q) for q in outs], _vp(stream)))


def grid_fill(u, v, valid, domain, radius, min_neighbours, max_passes, device=0):
    """``sid_grid_fill`` on host arrays: u, v float64 [rows, cols], valid and domain uint8 [rows, cols] or None (C-contiguous)
    -> u_out, v_out float64 [rows, cols], gen int32 [rows, cols].  device=-1: the kernels' source in a host loop (tests)."""
    rows, cols = u.shape
    uo, vo = np.empty((rows, cols), dtype=np.float64), np.empty((rows, cols), dtype=np.float64)
    gen = np.empty((rows, cols), dtype=np.int32)
    _grid_check(lib().sid_grid_fill(int(device), _p(u, _f64p), _p(v, _f64p), _opt_u8(valid), _opt_u8(domain), rows, cols,
                                    int(radius), int(min_neighbours), int(max_passes), _p(uo, _f64p), _p(vo, _f64p),
                                    _p(gen, _i32p)))
    return uo, vo, gen


def grid_fill_device(u, v, valid, domain, rows, cols, radius, min_neighbours, max_passes, u_out, v_out, gen, stream):
    """``sid_grid_fill_device`` on raw device pointers (torch ``data_ptr()``; valid, domain 0 for none)."""
    _grid_check(lib().sid_grid_fill_device(*[_vp(q) for q in (u, v, valid, domain)], int(rows), int(cols), int(radius),
                                           int(min_neighbours), int(max_passes), _vp(u_out), _vp(v_out), _vp(gen),
                                           _vp(stream)))


def grid_smooth(u, v, valid, weights, radius, device=0):
    """``sid_grid_smooth`` on host arrays: u, v float64 [rows, cols], valid uint8 or None, weights float64
    [2 radius + 1, 2 radius + 1] (C-contiguous all) -> u_out, v_out float64 [rows, cols].  device=-1: the host loop (tests)."""
    rows, cols = u.shape
    uo, vo = np.empty((rows, cols), dtype=np.float64), np.empty((rows, cols), dtype=np.float64)
    _grid_check(lib().sid_grid_smooth(int(device), _p(u, _f64p), _p(v, _f64p), _opt_u8(valid), rows, cols, _p(weights, _f64p),
                                      int(radius), _p(uo, _f64p), _p(vo, _f64p)))
    return uo, vo


def grid_smooth_device(u, v, valid, rows, cols, weights, radius, u_out, v_out, stream):
    """``sid_grid_smooth_device`` on raw device pointers; `weights` is a host float64 array (it travels as a kernel argument)."""
    _grid_check(lib().sid_grid_smooth_device(*[_vp(q) for q in (u, v, valid)], int(rows), int(cols), _p(weights, _f64p),
                                             int(radius), _vp(u_out), _vp(v_out), _vp(stream)))


def warp_image(x, y, xs, ys, valid, src, dtype, src_shape, out_shape, order, fill, diagonal, flags, want_out, want_covered,
               want_maps, device=0):
    """``sid_warp_image`` on host arrays: x, y, xs, ys float64 [R, C] and valid uint8 or None (C-contiguous); src a 2-D
    array of `dtype` ('uint8' or 'float32') with unit inner stride, or None; -> out, covered, map_x, map_y (None where not
    wanted).  device=-1: the kernels' source in a host loop (tests)."""
    rows, cols = x.shape
    ro, co = int(out_shape[0]), int(out_shape[1])
    out = np.empty((ro, co), dtype=dtype) if want_out else None
    covered = np.empty((ro, co), dtype=np.uint8) if want_covered else None
    map_x = np.empty((ro, co), dtype=np.float32) if want_maps else None
    map_y = np.empty((ro, co), dtype=np.float32) if want_maps else None
    stride = src.strides[0] // src.itemsize if src is not None and src.shape[0] > 1 else int(src_shape[1])
    _warp_check(lib().sid_warp_image(int(device), *[_p(a, _f64p) for a in (x, y, xs, ys)], _opt_u8(valid), rows, cols,
                                     _vp(src), WARP_DTYPES[dtype], int(src_shape[0]), int(src_shape[1]), stride, ro, co,
                                     int(order), float(fill), int(diagonal), int(flags), _vp(out), co, _vp(covered),
                                     _vp(map_x), _vp(map_y)))
    return out, covered, map_x, map_y


def warp_image_device(x, y, xs, ys, valid, rows, cols, src, dtype, src_shape, src_stride, out_shape, order, fill, diagonal,
                      flags, out, out_stride, covered, map_x, map_y, stream):
    """``sid_warp_image_device`` on raw device pointers (torch ``data_ptr()``; 0 for none)."""
    vp = [_vp(q) for q in (x, y, xs, ys, valid, src, out, covered, map_x, map_y)]
    _warp_check(lib().sid_warp_image_device(*vp[:5], int(rows), int(cols), vp[5], WARP_DTYPES[dtype], int(src_shape[0]),
                                            int(src_shape[1]), int(src_stride), int(out_shape[0]), int(out_shape[1]),
                                            int(order), float(fill), int(diagonal), int(flags), vp[6], int(out_stride),
                                            vp[7], vp[8], vp[9], _vp(stream)))


def track_points(x, y, xs, ys, valid, diagonal, flags, px, py, want_tri=False, device=0):
    """``sid_track_points`` on host arrays: x, y, xs, ys float64 [R, C] and valid uint8 or None, px, py float64 [n]
    (C-contiguous all) -> sx, sy float64 [n], tri int32 [n] (None when not wanted).  device=-1: the kernels' source in a host
    loop (tests)."""
    rows, cols = x.shape
    n = int(px.shape[0])
    sx, sy = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
    tri = np.empty(n, dtype=np.int32) if want_tri else None
    if n:                                                                # (an empty array has no address to hand over)
        _track_check(lib().sid_track_points(int(device), *[_vp(a.ctypes.data or 1) for a in (x, y, xs, ys)], _vp(valid), rows, cols,
                                            int(diagonal), int(flags), _vp(px), _vp(py), n, _vp(sx), _vp(sy), _vp(tri)))
    return sx, sy, tri


def track_points_device(x, y, xs, ys, valid, rows, cols, diagonal, flags, px, py, n, sx, sy, tri, stream):
    """``sid_track_points_device`` on raw device pointers (torch ``data_ptr()``; valid, tri 0 for none)."""
    _track_check(lib().sid_track_points_device(*[_vp(q) for q in (x, y, xs, ys, valid)], int(rows), int(cols), int(diagonal),
                                               int(flags), _vp(px), _vp(py), int(n), _vp(sx), _vp(sy), _vp(tri), _vp(stream)))


def _corr_outputs(shape, want_r, want_count, want_sums):
    return (np.empty(shape, dtype=np.float64) if want_r else None, np.empty(shape, dtype=np.int32) if want_count else None,
            np.empty(tuple(shape) + (5,), dtype=np.int64) if want_sums else None)


def _row_stride(img):
    """Row stride in elements of a 2-D uint8 array with unit inner stride (a single row or no row: its length)."""
    return img.strides[0] if img.shape[0] > 1 and img.shape[1] > 0 else max(int(img.shape[1]), 0)


def corr_lattice(a, b, w, r0, c0, sr, sc, nr, nc, min_count, want_r=True, want_count=False, want_sums=False, device=0):
    """``sid_corr_lattice`` on host arrays: a, b uint8 [rows, cols] with unit inner stride -> r float64 [nr, nc], count int32
    [nr, nc], sums int64 [nr, nc, 5] (None where not wanted).  device=-1: the kernels' source in a host loop (tests)."""
    rows, cols = a.shape
    r, count, sums = _corr_outputs((int(nr), int(nc)), want_r, want_count, want_sums)
    if int(nr) * int(nc) == 0 and min(int(nr), int(nc)) >= 0:            # (an empty array has no address to hand over)
        return r, count, sums
    _corr_check(lib().sid_corr_lattice(int(device), _vp(a.ctypes.data or 1), _row_stride(a), _vp(b.ctypes.data or 1), _row_stride(b),
                                       rows, cols, int(w), int(r0), int(c0), int(sr), int(sc), int(nr), int(nc), int(min_count),
                                       _vp(r), _vp(count), _vp(sums)))
    return r, count, sums


def corr_points(a, b, w, c, r, valid, min_count, want_r=True, want_count=False, want_sums=False, device=0):
    """``sid_corr_points`` on host arrays: a, b as above; c, r int32 [n] and valid uint8 [n] or None (C-contiguous)
    -> r float64 [n], count int32 [n], sums int64 [n, 5] (None where not wanted)."""
    rows, cols = a.shape
    n = int(c.shape[0])
    out, count, sums = _corr_outputs((n,), want_r, want_count, want_sums)
    if n == 0:
        return out, count, sums
    _corr_check(lib().sid_corr_points(int(device), _vp(a.ctypes.data or 1), _row_stride(a), _vp(b.ctypes.data or 1), _row_stride(b),
                                      rows, cols, int(w), _vp(c), _vp(r), _vp(valid), n, int(min_count), _vp(out), _vp(count),
                                      _vp(sums)))
    return out, count, sums


def corr_lattice_device(a, a_stride, b, b_stride, rows, cols, w, r0, c0, sr, sc, nr, nc, min_count, r, count, sums, stream):
    """``sid_corr_lattice_device`` on raw device pointers (torch ``data_ptr()``; 0 for an output that is not wanted)."""
    _corr_check(lib().sid_corr_lattice_device(_vp(a), int(a_stride), _vp(b), int(b_stride), int(rows), int(cols), int(w), int(r0),
                                              int(c0), int(sr), int(sc), int(nr), int(nc), int(min_count), _vp(r), _vp(count),
                                              _vp(sums), _vp(stream)))


def corr_points_device(a, a_stride, b, b_stride, rows, cols, w, c, r, valid, npts, min_count, out, count, sums, stream):
    """``sid_corr_points_device`` on raw device pointers (valid 0 for none)."""
    _corr_check(lib().sid_corr_points_device(_vp(a), int(a_stride), _vp(b), int(b_stride), int(rows), int(cols), int(w), _vp(c),
                                             _vp(r), _vp(valid), int(npts), int(min_count), _vp(out), _vp(count), _vp(sums),
                                             _vp(stream)))


def _prep_coeffs(coeffs):
    if coeffs is None:
        return None, None
    c = np.ascontiguousarray(coeffs, dtype=np.float64)
    if c.shape != (6,):
        raise ValueError('six float64 coefficients expected (col, col^2, row, row^2, col*row, 1), got shape %s' % (c.shape,))
    return c, _p(c, _f64p)


def prep_subsample(img, rows, cols, stride, ia, mask, dB, hh_factor, step, sub_ptr, stream=0):
    """``sid_prep_subsample`` on raw device pointers: ``img`` a pointer, ``ia`` / ``mask`` (pointer, row stride) or None."""
    ia_ptr, ia_stride = ia if ia is not None else (0, 0)
    m_ptr, m_stride = mask if mask is not None else (0, 0)
    _prep_check(lib().sid_prep_subsample(_vp(img), rows, cols, stride, _vp(ia_ptr), ia_stride,
                                         _vp(m_ptr), m_stride, int(bool(dB)), float(hh_factor), int(step),
                                         _vp(sub_ptr), _vp(stream)))


def prep_apply(img, rows, cols, stride, ia, mask, dB, hh_factor, coeffs, out_ptr, out_stride, stream=0):
    """``sid_prep_apply`` on raw device pointers; ``coeffs``: six float64 (host) or None for no detrend."""
    ia_ptr, ia_stride = ia if ia is not None else (0, 0)
    m_ptr, m_stride = mask if mask is not None else (0, 0)
    keep, cp = _prep_coeffs(coeffs)
    _prep_check(lib().sid_prep_apply(_vp(img), rows, cols, stride, _vp(ia_ptr), ia_stride,
                                     _vp(m_ptr), m_stride, int(bool(dB)), float(hh_factor), cp,
                                     _vp(out_ptr), out_stride, _vp(stream)))


def prep_spatial_mean(rows, cols, coeffs, out_ptr, out_stride, stream=0):
    """``sid_prep_spatial_mean``: the float64 polynomial image for six coefficients, into a device buffer."""
    keep, cp = _prep_coeffs(coeffs)
    if cp is None:
        raise ValueError('six float64 coefficients expected')
    _prep_check(lib().sid_prep_spatial_mean(rows, cols, cp, _vp(out_ptr), out_stride, _vp(stream)))


def prep_debug_log10(first_bits, n):
    """``sid_prep_debug_log10``: (mismatches, library-route evaluations) of the dB step's float32 logarithm against
    float(log10(double(x))) over the ``n`` float32 bit patterns from ``first_bits`` on."""
    counts = (C.c_uint64 * 2)()
    _prep_check(lib().sid_prep_debug_log10(int(first_bits), int(n), counts))
    return int(counts[0]), int(counts[1])


def mask_workspace_bytes(h, w):
    """``sid_mask_workspace_bytes``: device scratch for a water mask of ``h`` x ``w``."""
    return int(lib().sid_mask_workspace_bytes(int(h), int(w)))


def mask_landmask(wm, h, w, H, W, work_ptr, mask, wmz, stream=0):
    """``sid_mask_landmask`` on raw device pointers: ``wm`` / ``mask`` / ``wmz`` are (pointer, row stride), the last two or None."""
    m_ptr, m_stride = mask if mask is not None else (0, 0)
    z_ptr, z_stride = wmz if wmz is not None else (0, 0)
    _mask_check(lib().sid_mask_landmask(_vp(wm[0]), int(h), int(w), int(wm[1]), int(H), int(W), _vp(work_ptr), _vp(m_ptr), m_stride,
                                        _vp(z_ptr), z_stride, _vp(stream)))


def mask_invalid(wm, h, w, H, W, work_ptr, img, dB, ia, hh_factor, mask, wmz=None, stream=0):
    """``sid_mask_invalid`` on raw device pointers: ``img`` / ``mask`` are (pointer, row stride); ``wm`` (with ``h``, ``w``, ``work_ptr``),
    ``ia`` and ``wmz`` are (pointer, row stride) or None."""
    w_ptr, w_stride = wm if wm is not None else (0, 0)
    ia_ptr, ia_stride = ia if ia is not None else (0, 0)
    z_ptr, z_stride = wmz if wmz is not None else (0, 0)
    _mask_check(lib().sid_mask_invalid(_vp(w_ptr), int(h), int(w), int(w_stride), int(H), int(W), _vp(work_ptr), _vp(img[0]), int(img[1]),
                                       int(bool(dB)), _vp(ia_ptr), int(ia_stride), float(hh_factor), _vp(mask[0]), int(mask[1]),
                                       _vp(z_ptr), int(z_stride), _vp(stream)))


def resize(src, dtype, rows, cols, stride, dst, out_rows, out_cols, dst_stride, option, stream=0):
    """``sid_resize_f32`` (``dtype`` 'float32'; ``option``: nan_omit) or ``sid_resize_u8`` ('uint8'; ``option``: zero_invalid) on raw
    device pointers."""
    fn = {'float32': lib().sid_resize_f32, 'uint8': lib().sid_resize_u8}[dtype]
    _resize_check(fn(_vp(src), int(rows), int(cols), int(stride), _vp(dst), int(out_rows), int(out_cols), int(dst_stride),
                     int(bool(option)), _vp(stream)))


def resize_prep_apply(img, rows, cols, stride, ia, mask, dB, hh_factor, coeffs, out_ptr, out_rows, out_cols, out_stride, stream=0):
    """``sid_resize_prep_apply`` on raw device pointers: ``prep_apply`` of the image and incidence angle averaged down to
    ``out_rows`` x ``out_cols``; ``mask`` (pointer, row stride) has that shape."""
    ia_ptr, ia_stride = ia if ia is not None else (0, 0)
    m_ptr, m_stride = mask if mask is not None else (0, 0)
    keep, cp = _prep_coeffs(coeffs)
    _resize_check(lib().sid_resize_prep_apply(_vp(img), int(rows), int(cols), int(stride), _vp(ia_ptr), int(ia_stride),
                                              _vp(m_ptr), int(m_stride), int(bool(dB)), float(hh_factor), cp,
                                              _vp(out_ptr), int(out_rows), int(out_cols), int(out_stride), _vp(stream)))


def resize_prep_subsample(img, rows, cols, stride, ia, mask, dB, hh_factor, step, out_rows, out_cols, sub_ptr, stream=0):
    """``sid_resize_prep_subsample`` on raw device pointers: ``prep_subsample`` of the same reduced images."""
    ia_ptr, ia_stride = ia if ia is not None else (0, 0)
    m_ptr, m_stride = mask if mask is not None else (0, 0)
    _resize_check(lib().sid_resize_prep_subsample(_vp(img), int(rows), int(cols), int(stride), _vp(ia_ptr), int(ia_stride),
                                                  _vp(m_ptr), int(m_stride), int(bool(dB)), float(hh_factor), int(step),
                                                  int(out_rows), int(out_cols), _vp(sub_ptr), _vp(stream)))
