"""A batched auto-reset simulator in torch, for the device-actor tests: E point
masses in the plane, each pushed by its 2-D action towards its own goal.  It is
deterministic (two instances built alike stay alike, bit for bit) and lives on
whatever device it is given.

Observation [E][8] float32: position (2), velocity (2), goal - position (2), the
episode clock as a fraction of the env's episode length, 1.  Reward float64 [E]:
minus the distance to the goal.  Env e's episodes last 2 + e % 5 steps, so resets
fall at different steps; the ends of envs with e % 3 == 0 are time limits
(done = 1, terminated = 0), the others true terminations.  An env whose episode
ends resets itself: the observation returned with done = 1 is the first of its
next episode, which starts where a counter of that env's episodes puts it."""
import torch

N_OBS, N_ACT = 8, 2


class StubDeviceSim:
    def __init__(self, E, device):
        self.E, self.device = int(E), torch.device(device)
        e = torch.arange(self.E, device=self.device)
        self.length = 2 + e % 5
        self.time_limit = e % 3 == 0
        self.goal = torch.stack([torch.cos(0.7 * e), torch.sin(1.3 * e)], dim=1).float()
        self.episode = torch.zeros(self.E, dtype=torch.int64, device=self.device)
        self.clock = torch.zeros(self.E, dtype=torch.int64, device=self.device)
        self.pos = torch.zeros((self.E, 2), dtype=torch.float32, device=self.device)
        self.vel = torch.zeros((self.E, 2), dtype=torch.float32, device=self.device)
        self._start(torch.ones(self.E, dtype=torch.bool, device=self.device))

    def _start(self, mask):
        e = torch.arange(self.E, device=self.device)
        k = (e + 3 * self.episode).float()
        start = 0.5 * torch.stack([torch.sin(0.9 * k), torch.cos(0.4 * k)], dim=1)
        self.pos = torch.where(mask[:, None], start, self.pos)
        self.vel = torch.where(mask[:, None], torch.zeros_like(self.vel), self.vel)
        self.clock = torch.where(mask, torch.zeros_like(self.clock), self.clock)

    def observe(self):
        frac = (self.clock.float() / self.length.float())[:, None]
        return torch.cat([self.pos, self.vel, self.goal - self.pos, frac, torch.ones_like(frac)], dim=1).contiguous()

    def step(self, actions):
        """(observations [E][8] f32, rewards [E] f64, done [E] u8, terminated [E] u8)"""
        a = actions.float().clamp(-1.0, 1.0)
        self.vel = 0.9 * self.vel + 0.1 * a
        self.pos = self.pos + 0.1 * self.vel
        rewards = -(self.goal - self.pos).double().norm(dim=1)
        self.clock = self.clock + 1
        done = self.clock >= self.length
        terminated = done & ~self.time_limit
        self.episode = self.episode + done.long()
        self._start(done)
        return self.observe(), rewards, done.to(torch.uint8), terminated.to(torch.uint8)
