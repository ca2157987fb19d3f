"""How many matrices of a batch are still live in each outer iteration of the rank-r solver.

Runs bench.py (same arguments, e.g. `--workload cfg3 --steps 1 --warmup 0`) with
RankRSolver's filter wrapped: every outer iteration starts with one _filter call, and the
mask it is given (self._active, 1 = live) is summed there.  The read-back synchronises, so
the throughput such a run prints means nothing; the counts are exact.  One line per solve
call, then the totals: outer iterations, those with a frozen set, and the frozen share of
their batch-wide work.

    python tools/live_count.py --workload cfg2 --steps 1 --warmup 0 --no-api-path
"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ee274_convexcaldera_llm_quantization_amd import solver as S  # noqa: E402

_calls = []          # one record per solve call: [B, cold, [live per outer iteration]]
_in_segments = [0]

_filter = S.RankRSolver._filter
_more = S.RankRSolver._more_segments
_solve_iter = S.RankRSolver.solve_iter


def filter_counted(self, X, coef, single=False, keep=()):
    if not _in_segments[0] and getattr(self, "_lc_rec", None) is not None:
        self._lc_rec[2].append(int(self._active.sum().item()))
    return _filter(self, X, coef, single=single, keep=keep)


def more_counted(self, *a, **kw):
    _in_segments[0] += 1
    try:
        return _more(self, *a, **kw)
    finally:
        _in_segments[0] -= 1


def solve_iter_counted(self, Y, warm=True, **kw):
    self._lc_rec = [self.B, not (warm and self.X is not None), []]
    _calls.append(self._lc_rec)
    return (yield from _solve_iter(self, Y, warm, **kw))


S.RankRSolver._filter = filter_counted
S.RankRSolver._more_segments = more_counted
S.RankRSolver.solve_iter = solve_iter_counted


def report():
    outer = frozen_iters = 0
    work = skipped = 0
    for i, (B, cold, live) in enumerate(_calls):
        print(f"live_count: call {i:4d} B={B:4d} {'cold' if cold else 'warm'} live per outer iteration: {live}")
        outer += len(live)
        frozen_iters += sum(1 for v in live if v < B)
        work += B * len(live)
        skipped += sum(B - v for v in live)
    print(f"live_count: {len(_calls)} solve calls, {outer} outer iterations, {frozen_iters} with a frozen set; "
          f"frozen share of the batch-wide work {skipped}/{work} = {100.0 * skipped / max(1, work):.2f} %")


if __name__ == "__main__":
    sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
    try:
        runpy.run_path(sys.argv[0], run_name="__main__")
    finally:
        report()
