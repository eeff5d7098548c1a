from . import dicl, raft  # noqa: F401
