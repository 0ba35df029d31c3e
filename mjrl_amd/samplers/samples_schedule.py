"""Which trajectories a lock-stepped sampler starts, and when it stops, for
sample_mode="samples" (mjrl/samplers/batch_sampler.py:58-103 on one core).

The reference collects trajectory after trajectory (trajectory k is the rollout
seeded s0 + k) `while sampled_so_far < N`: the batch is the shortest prefix 0..K
whose lengths sum to >= N.  A lock-stepped sampler runs S trajectories at once
and learns their lengths only as they end, so it has to start some it will not
keep.  The rule, held here so that the in-process loop (vector_sampler.py) and
the worker loop (env_workers.py) cannot differ:

  - trajectories start in index order;
  - none starts once the rows of the finished trajectories plus the current
    lengths of the live ones reach N: lengths only grow, so the prefix that
    reaches N ends among those already started (K cannot be larger);
  - sampling stops at the first moment trajectories 0..K have all ended with a
    prefix sum >= N; live trajectories with an index above K are abandoned
    (finished ones above K are simply not returned).

Pure Python: no numpy, no torch, no GPU.
"""


class SamplesSchedule:
    """N: the number of timesteps asked for.  The sampler calls start() for a
    free slot while may_start(), step(k) for every row trajectory k records,
    end(k) when it ends, and stops when `done`."""

    def __init__(self, N):
        self.N = int(N)
        self.length = []     # rows recorded so far, by trajectory index
        self.ended = []
        self.rows = 0        # rows of every started trajectory, finished or live
        self.closed = 0      # trajectories 0..closed-1 have ended ...
        self.prefix = 0      # ... with this many rows
        self.K = None        # the last accepted index, once known

    @property
    def done(self):
        return self.K is not None or self.N <= 0

    @property
    def accepted(self):
        """The number of trajectories returned (K + 1); 0 for N <= 0."""
        return 0 if self.K is None else self.K + 1

    def may_start(self):
        return not self.done and self.rows < self.N

    def start(self):
        """The index of the trajectory that starts now."""
        if not self.may_start():
            raise RuntimeError("SamplesSchedule.start: %d of %d rows are already started" % (self.rows, self.N))
        self.length.append(0)
        self.ended.append(False)
        return len(self.length) - 1

    def step(self, k):
        self.length[k] += 1
        self.rows += 1

    def end(self, k):
        self.ended[k] = True
        while self.K is None and self.closed < len(self.ended) and self.ended[self.closed]:
            self.prefix += self.length[self.closed]
            if self.prefix >= self.N:
                self.K = self.closed
            self.closed += 1

    def abandoned(self):
        """Once done: the started trajectories that are still live (all above K)."""
        return [k for k in range(self.accepted, len(self.ended)) if not self.ended[k]]
