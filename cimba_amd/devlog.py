"""Device log stream: format and replay the records a logged model returns.

A model that opts in (``Cfg::DEVICE_LOG``) returns ``log_records`` (a
structured array of the surviving records, sorted by ``(trial, seq)``),
``log_emitted`` and ``log_first``.  The functions here turn them into the
logger's lines — ``[trial] [seed] time who tag: name value=v`` — through
the one native formatter.

    r = cimba_amd.mm1log_gpu(ntrials=1024, num_objects=100, seed=7,
                             log_first=17, log_count=1)
    print("\\n".join(devlog.format_lines(r, name="mm1log", seed=7)))
"""
from . import _C


def format_lines(result, name, seed):
    """One logger line per record of ``result["log_records"]``.

    ``name`` is the registered model name (it selects the record names),
    ``seed`` the master seed of the run (each line prints its trial's
    derived seed, as the host logger does)."""
    return list(_C.devlog_format(result["log_records"], seed, name))


def replay(result, name, seed):
    """Print the records through the host logger, whose current flag mask
    (``logger_flags_on`` / ``logger_flags_off``) and stream apply.  Returns
    the number of records walked."""
    return _C.devlog_replay(result["log_records"], result["log_emitted"],
                            result["log_first"], seed, name)
