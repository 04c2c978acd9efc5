"""Inference CLI of the continuous (CNF) model - the reference's `modules/continuous/upsample.py` (identical to the
discrete script except for the model class, `continuous/upsample.py:15,29`):

  python -m puflow_amd.upsample_cnf --source=in/ --target=out/ --checkpoint=puflow-x4-cnf-pu1k.pt --up_ratio=4

Not in the reference - a frozen step schedule: `--record_schedule FILE [--schedule_refine M]` records the adaptive
solver's accepted steps on the first pass, writes them to FILE and integrates every pass on them (one launch per integration);
`--schedule FILE` loads such a file.
"""
from __future__ import annotations

from . import upsample
from .cnf import PointInterpFlow, load_schedule


def _add_arguments(parser) -> None:
    parser.add_argument("--schedule", type=str, default=None, metavar="FILE",
                        help="(not in the reference) integrate on the frozen step schedule in FILE instead of adaptively")
    parser.add_argument("--record_schedule", type=str, default=None, metavar="FILE",
                        help="(not in the reference) record the adaptive solver's accepted steps on the first pass, write them to "
                             "FILE and integrate on them from that pass on")
    parser.add_argument("--schedule_refine", type=int, default=1, metavar="M", help="cut every recorded step into M parts")


def _setup(network: PointInterpFlow, args) -> None:
    if args.schedule is not None and args.record_schedule is not None:
        raise SystemExit("--schedule and --record_schedule exclude each other")
    if args.schedule is not None:
        network.step_schedule = load_schedule(args.schedule)
    if args.record_schedule is not None:
        network.record_first = (args.record_schedule, int(args.schedule_refine))


def main(argv=None):
    upsample.main(argv, network_cls=PointInterpFlow, add_arguments=_add_arguments, network_setup=_setup)


if __name__ == "__main__":
    main()
