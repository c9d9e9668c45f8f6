"""Plan streams for the scripts' command lines: --streams R [--tail K] (include/eirgrid_hip.h eg_plan_streams_set, Engine.set_streams).

A script adds the two options to its parser with add_stream_arguments and puts them on its engine with apply_streams, next to
constraints.add_constraint_arguments / apply_constraints: every plan batch the script then runs is judged over R draw streams and
ranks, picks and reports committed outcomes — the mean of the K worst streams, K = R by default."""
from __future__ import annotations

STREAMS_MAX = 64      # EG_STREAMS_MAX


def add_stream_arguments(parser) -> None:
    """--streams R and --tail K for a script's argparse parser; apply_streams puts them on the engine"""
    parser.add_argument("--streams", type=int, default=0, metavar="R",
                        help=f"judge every plan over R draw streams, 2..{STREAMS_MAX}: the seeds of R consecutive episode indices (default: one stream)")
    parser.add_argument("--tail", type=int, default=None, metavar="K",
                        help="with --streams: commit the mean of the K worst streams, 1..R (default R, the mean outcome; 1: the worst stream)")


def apply_streams(engine, args, cost_only=None) -> int:
    """the --streams / --tail of `args` set on `engine` (none given: nothing is set); the streams are ordered by the score the script
    ranks by: `cost_only`, or the script's own --cost-only when it has one.  Returns R (0: no streams)."""
    if args.tail is not None and args.streams < 2:
        raise SystemExit("--tail needs --streams R with R >= 2")
    if args.streams in (0, 1):
        return 0
    if cost_only is None:
        cost_only = bool(getattr(args, "cost_only", False))
    engine.set_streams(args.streams, args.tail, cost_only)      # (the library's own refusal names what is out of range)
    return args.streams
