"""MI355X-native pattern-matching (PM) hot path of sea_ice_drift.

Only the per-grid-point rotated-template MCC sweep is implemented here (as a HIP kernel
for gfx950 behind the C ABI of include/sid_pm.h) together with the host-side callers that
keep the reference's call shape: ``pattern_matching`` and ``SeaIceDrift.get_drift_PM``.

Beside it, not the reference's: ``libfilter``, ``libdefor``, ``libwarp`` (``warp_image``) and ``libcorr``
(``local_correlation``, ``local_correlation_at``: the local correlation of two uint8 images, e.g. of image 1 with
the warped image 2) and ``libtrack`` (``map_points``, ``advect``, ``round_trip``: arbitrary points carried through a
drift grid).
"""
__version__ = '0.1.0'
