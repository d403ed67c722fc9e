"""Snapshot metrics (the reference's ``metrics/`` package by module name): ``metric_main`` is the registry and the report
format, ``metric_utils`` the options and the two HIP statistics, ``reconstruction`` the paired-reconstruction metric."""
