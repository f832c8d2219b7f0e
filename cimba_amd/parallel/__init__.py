from .experiment import (  # noqa: F401
    allreduce_datasummary,
    allreduce_histogram,
    allreduce_wtdsummary,
    run_distributed_mm1,
    shard_range,
)
