"""MI355X-native offline ICM sweep: ctypes binding (`_lib`) and host driver (`engine`)."""
from .engine import IcmError, SweepEngine, bearing_tables, cluster_first_scan, filtrar_map, prefilter_scans, seed_first_scan  # noqa: F401
from .batch import init_pass_batch, run_offline, sweep_batch  # noqa: F401
