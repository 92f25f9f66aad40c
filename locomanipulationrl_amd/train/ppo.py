"""Compact PPO with the hyper-parameters and semantics the reference's skrl scripts configure
(scripts/skrl_ppo_locomotion.py:86-112: rollouts 48, 5 epochs, 1 mini-batch, gamma 0.99, lambda 0.95, lr 3e-4 with
KL-adaptive schedule (threshold 0.012), grad-norm clip 1.0, ratio clip 0.2, value clip 0.2 with clipped predictions,
entropy scale 0, value scale 1, RunningStandardScaler on observations and values).

skrl itself is third-party and not installed here; this trainer exists so that the engine can be accepted
*behaviourally* (the task's success rate rises under the reference's PPO recipe) and to exercise the multi-GPU
exchange of SURVEY 8(e): rollout returns / advantages are all-gathered over RCCL for global advantage normalisation and
the gradients are all-reduced.  Rollouts use the matrix-core policy forward (csrc/lm_policy.hip); updates use autograd, or - opt-in - the
fused loss-gradient kernels and the GAE kernel: PPO(hip_update=True) for the SharedMLP (csrc/lm_ppo.hip),
PPO(gnn_hip_update=True) for the GraphPolicy (csrc/lm_gnn_ppo.hip).  With either of them, PPO(hip_optimizer=True) also runs the gradient-norm
clip, Adam and the KL-adaptive rate on the device (csrc/lm_optim.hip): the epoch loop then holds no torch optimiser launch and no host wait.
PPO(hip_prepare=True) moves the rest there too (csrc/lm_prepare.hip): the parameter pack of the rollout's forward kernel, both running scalers and
the normalisation of the batch; with hip_optimizer as well, update(last_value, fetch=False) is a fixed sequence of launches with no host wait.
"""
from __future__ import annotations

import math
import time
from typing import Dict

import torch
import torch.distributed as dist

from .. import distributed as D


class RunningStandardScaler:
    """skrl.resources.preprocessors.torch.RunningStandardScaler: running mean/variance, (x-mean)/(sqrt(var)+eps), clip 5.
    device_block=True: mean, var and count are views of ONE float64 block `state` = mean | var | count, which the kernels of csrc/lm_prepare.hip
    read and update in place (update() and load_state_dict() then write through the views); everything else behaves the same."""

    def __init__(self, size: int, device, epsilon: float = 1e-8, clip: float = 5.0, device_block: bool = False):
        self.state = None
        if device_block:
            self.state = torch.zeros(2 * size + 1, device=device, dtype=torch.float64); self.state[size:] = 1.0
            self.mean, self.var, self.count = self.state[:size], self.state[size:2 * size], self.state[2 * size]
        else:
            self.mean = torch.zeros(size, device=device, dtype=torch.float64)
            self.var = torch.ones(size, device=device, dtype=torch.float64)
            self.count = torch.ones((), device=device, dtype=torch.float64)
        self.eps, self.clip = epsilon, clip

    def _set(self, mean, var, count):
        if self.state is None:
            self.mean, self.var, self.count = mean, var, count
        else:
            self.mean.copy_(mean); self.var.copy_(var); self.count.copy_(count)

    def update(self, x: torch.Tensor):
        x = x.reshape(-1, self.mean.numel()).double()
        n = torch.tensor(float(x.shape[0]), device=x.device, dtype=torch.float64)
        s, ss = x.sum(0), (x * x).sum(0)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            buf = torch.cat((s, ss, n.view(1))); dist.all_reduce(buf); s, ss, n = buf[:s.numel()], buf[s.numel():-1], buf[-1]
        bmean = s / n; bvar = (ss / n - bmean * bmean).clamp_min(0) * n / (n - 1).clamp_min(1)
        delta = bmean - self.mean; tot = self.count + n
        m2 = self.var * self.count + bvar * n + delta * delta * self.count * n / tot
        self._set(self.mean + delta * n / tot, m2 / tot, tot)

    def state_dict(self):
        return {"mean": self.mean.detach().cpu().clone(), "var": self.var.detach().cpu().clone(), "count": self.count.detach().cpu().clone()}

    def load_state_dict(self, sd):
        dev = self.mean.device
        assert tuple(sd["mean"].shape) == tuple(self.mean.shape), (tuple(sd["mean"].shape), tuple(self.mean.shape))
        self._set(*(sd[k].to(dev, torch.float64).clone() for k in ("mean", "var", "count")))

    def __call__(self, x: torch.Tensor, inverse: bool = False):
        mean, std = self.mean.float(), self.var.float().sqrt()
        if inverse:
            return std * torch.clamp(x, -self.clip, self.clip) + mean
        return torch.clamp((x - mean) / (std + self.eps), -self.clip, self.clip)


def gaussian_logp(mean, log_std, act):
    return (-0.5 * ((act - mean) / log_std.exp()) ** 2 - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)


def ppo_loss(model_outputs, act, old_logp, old_val_n, adv, ret_n, rclip, vclip, vscale, escale):
    """The loss of one PPO mini-batch (skrl PPO._update with clipped predictions): model_outputs = (mean, log_std, v) of the model on the
    normalised observations.  Returns (loss, loss_pi, loss_v, kl, ent); kl carries no gradient.  Dtype-agnostic: update() calls it in
    float32, the tests of the HIP update in float64 as their reference."""
    mean, log_std, v = model_outputs
    logp = gaussian_logp(mean, log_std, act)
    ratio_log = logp - old_logp
    with torch.no_grad():
        kl = ((ratio_log.exp() - 1) - ratio_log).mean()
    ratio = ratio_log.exp()
    surr = torch.min(adv * ratio, adv * ratio.clamp(1 - rclip, 1 + rclip))
    v = v.squeeze(-1); v = old_val_n + (v - old_val_n).clamp(-vclip, vclip)
    loss_pi = -surr.mean(); loss_v = vscale * torch.nn.functional.mse_loss(ret_n, v)
    ent = (log_std + 0.5 + 0.5 * math.log(2 * math.pi)).sum()
    loss = loss_pi + loss_v - escale * ent
    return loss, loss_pi, loss_v, kl, ent


class PPO:
    def __init__(self, env, model, rollouts=48, learning_epochs=5, mini_batches=1, gamma=0.99, lam=0.95, lr=3e-4, kl_threshold=0.012,
                 grad_norm_clip=1.0, ratio_clip=0.2, value_clip=0.2, value_loss_scale=1.0, entropy_loss_scale=0.0, hip_inference=True,
                 fused_rollout=True, freeze_obs_scaler=False, max_lr=1e-2, min_log_std=None, hip_update=False, gnn_hip_update=False,
                 hip_optimizer=False, hip_prepare=False):
        """hip_prepare=True (with hip_update or gnn_hip_update, on a HIP device, one rank, a fused rollout): collect() packs the rollout's
        parameter block with one launch from the flat block and the observation scaler's state block (no model.refresh, no blocking read), and
        update() prepares the batch with the launches of csrc/lm_prepare.hip.  The packers' range check becomes a status word on the device: a
        weight that is not finite or not below 6e4 raises their ValueError at the next fetch (the next update(fetch=True), i.e. the next logged
        iteration of train(), or state_dict()), not at the collect() that met it."""
        self.env, self.model = env, model
        self.dev = next(model.parameters()).device
        self.phase_marks = None       # timing hook: see _mark
        self.hip_optimizer = bool(hip_optimizer)
        if self.hip_optimizer and not (hip_update or gnn_hip_update):
            raise ValueError("hip_optimizer=True steps the flat parameter blocks of a fused update: pass hip_update=True (SharedMLP) or gnn_hip_update=True "
                             "(GraphPolicy) as well")
        self.hip_prepare = bool(hip_prepare)
        if self.hip_prepare:
            if not (hip_update or gnn_hip_update):
                raise ValueError("hip_prepare=True packs the rollout's parameters from the flat block of a fused update: pass hip_update=True (SharedMLP) or "
                                 "gnn_hip_update=True (GraphPolicy) as well")
            if self.dev.type != "cuda" or not torch.cuda.is_available():
                raise ValueError(f"hip_prepare=True needs the model on a HIP device, not {self.dev} (the kernels have no CPU fallback)")
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError("hip_prepare=True runs on one rank: the all-reduce of the batch sums between lm_ppo_batch_stats and lm_ppo_batch_apply "
                                 "is not built yet (world > 1)")
        self.hip_update = bool(hip_update)
        if self.hip_update:
            # no CPU fallback and no quiet autograd path, as in lib.Engine: say why and stop
            n_in = int(env.observation_space.shape[0])
            if type(model).__name__ != "SharedMLP":
                raise ValueError(f"hip_update=True: the fused PPO gradient kernel is built for SharedMLP, not {type(model).__name__} (a GraphPolicy's fused update is gnn_hip_update=True)")
            if self.dev.type != "cuda" or not torch.cuda.is_available():
                raise ValueError(f"hip_update=True needs the model on a HIP device, not {self.dev} (the kernel has no CPU fallback)")
            if n_in not in (64, 88):
                raise ValueError(f"hip_update=True: the kernel is built for 64- and 88-wide observations, not {n_in}")
            from ..policies.mlp_model import bind_flat_params
            self._flat, self._gflat, self._offsets = bind_flat_params(model)      # parameters and .grads become views into two flat buffers
            self._ppo_stats = torch.zeros(4, device=self.dev); self._ws = {}
        self.gnn_hip_update = bool(gnn_hip_update)
        if self.gnn_hip_update:
            n_in = int(env.observation_space.shape[0])
            if self.hip_update:
                raise ValueError("gnn_hip_update=True and hip_update=True: one model, one fused update (hip_update is the SharedMLP's, gnn_hip_update the GraphPolicy's)")
            if type(model).__name__ != "GraphPolicy":
                raise ValueError(f"gnn_hip_update=True: the fused GNN gradient kernel is built for GraphPolicy, not {type(model).__name__} (hip_update=True is the SharedMLP's)")
            if self.dev.type != "cuda" or not torch.cuda.is_available():
                raise ValueError(f"gnn_hip_update=True needs the model on a HIP device, not {self.dev} (the kernel has no CPU fallback)")
            if n_in != 64:
                raise ValueError(f"gnn_hip_update=True: the GNN reads the 64-wide observation layout, not {n_in}")
            from ..policies.graph_model import bind_gnn_flat_params
            self._flat, self._gflat, self._offsets = bind_gnn_flat_params(model)      # parameters and .grads become views into two flat buffers
            self._ppo_stats = torch.zeros(4, device=self.dev); self._ws = {}
        self._fused_update = self.hip_update or self.gnn_hip_update
        self.N = env.num_envs
        self.T, self.epochs, self.mb = rollouts, learning_epochs, mini_batches
        self.gamma, self.lam, self.lr, self.kl_thr = gamma, lam, lr, kl_threshold
        self.gclip, self.rclip, self.vclip, self.vscale, self.escale = grad_norm_clip, ratio_clip, value_clip, value_loss_scale, entropy_loss_scale
        self.opt = torch.optim.Adam(model.parameters(), lr=lr)
        if self.hip_optimizer:
            # Adam's moments as two flat blocks laid out like the parameters, the rate and the step count in a device state block; self.opt
            # keeps the hyper-parameters and is the checkpoint format (filled from the blocks when saving, emptied into them when loading)
            from ..policies.optim import optim_state
            self._m, self._v = torch.zeros_like(self._flat), torch.zeros_like(self._flat)
            self._ostate = optim_state(self.dev, lr, 0)
            self._fetch = torch.zeros(self._ostate.numel() + 2 + int(self.hip_prepare), device=self.dev, dtype=torch.float64)      # + the pack status slot
            if self.hip_prepare: self._fetch[:self._ostate.numel()].copy_(self._ostate)      # the fetch block mirrors the state block between updates
            self._stats_all, self.last_kls = None, None
        self.freeze_obs_scaler = freeze_obs_scaler          # diagnostics: identity observation scaler (mean 0, var 1)
        self.max_lr, self.min_log_std = max_lr, min_log_std  # diagnostics: cap of the KL-adaptive rate (skrl: 1e-2); floor of log_std (skrl: -20)
        self.n_obs = int(env.observation_space.shape[0])          # 88 for the custom-controller tasks
        self.obs_scaler = RunningStandardScaler(self.n_obs, self.dev, device_block=self.hip_prepare)
        self.val_scaler = RunningStandardScaler(1, self.dev, device_block=self.hip_prepare)
        # MFMA forward kernels: MLP on the 64- and 88-wide observations, GNN on the 64-wide one
        self.hip = hip_inference and hasattr(model, "act_inference") and torch.cuda.is_available() and \
            (self.n_obs == 64 or (self.n_obs == 88 and type(model).__name__ == "SharedMLP"))
        z = lambda *s, dt=torch.float32: torch.zeros(*s, device=self.dev, dtype=dt)
        self.b_obs, self.b_act, self.b_logp = z(self.T, self.N, self.n_obs), z(self.T, self.N, 12), z(self.T, self.N)
        self.b_val, self.b_rew, self.b_done = z(self.T, self.N), z(self.T, self.N), z(self.T, self.N)
        self.world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        # fused rollout: forward -> sampling -> step x T as one hipGraph launch, buffers shared with the update
        self.rollout = None
        if self.hip and fused_rollout and hasattr(env, "_task") and hasattr(env._task, "make_rollout"):
            kind = "gnn" if type(model).__name__ == "GraphPolicy" else "mlp"
            model.refresh(self.dev, self.obs_scaler.mean.float(), self.obs_scaler.var.float(), self.obs_scaler.eps, self.obs_scaler.clip)
            self._packed = model._packed.clone(); self._log_std = model.log_std_parameter.detach().clone().float().contiguous()
            rank = dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0
            self.rollout = env._task.make_rollout(kind, self._packed, self._log_std, self.T, noise_seed=1000 + rank)
            ro = self.rollout
            self._ro_mode = "auto"      # one persistent kernel per rollout where the engine supports it and it pays, else the hipGraph replay
            self.b_obs, self.b_act, self.b_logp, self.b_rew = ro.obs[:self.T], ro.actions, ro.logp, ro.rewards
        if self.hip_prepare:
            if self.rollout is None:
                raise ValueError("hip_prepare=True packs straight into a fused rollout's parameter block: it needs hip_inference and fused_rollout on an "
                                 "engine task (env._task.make_rollout)")
            # the pack status: an int32 the pack kernel ORs into.  With hip_optimizer it is the low half of the last slot of the fetch block, so that
            # one copy brings the optimiser state, the losses and the status to the host
            self._pstatus = self._fetch[-1:].view(torch.int32)[:1] if self.hip_optimizer else torch.zeros(1, device=self.dev, dtype=torch.int32)
            self._kind = "gnn" if self.gnn_hip_update else "mlp"
            self._sums = torch.zeros(2 * self.n_obs + 5, device=self.dev, dtype=torch.float64); self._prep = {}

    # ------------------------------------------------------------------ policy evaluation
    def _policy(self, obs_raw):
        """mean, log_std, value (de-normalised) for raw observations; rollouts go through the MFMA forward."""
        with torch.no_grad():
            if self.hip:
                self.model.refresh(self.dev, self.obs_scaler.mean.float(), self.obs_scaler.var.float(), self.obs_scaler.eps, self.obs_scaler.clip)
                mean, log_std, v = self.model.act_inference(obs_raw.contiguous())
            else:
                mean, log_std, v = self.model(self.obs_scaler(obs_raw))
            return mean, log_std.detach(), self.val_scaler(v, inverse=True).squeeze(-1)

    _logp = staticmethod(gaussian_logp)

    # ------------------------------------------------------------------ one iteration = T env steps + update
    def collect(self, obs_raw):
        if self.rollout is not None:
            ro = self.rollout
            if self.hip_prepare:      # one launch, flat block + scaler block -> the plan's parameter block; the range check goes to self._pstatus
                from ..policies.prepare import pack_params
                pack_params(self._kind, self._flat, self.n_obs, self._packed, self._pstatus, self.obs_scaler.state, self.obs_scaler.eps, self.obs_scaler.clip)
                self._log_std.copy_(self.model.log_std_parameter.detach())
            else:
                self.model.refresh(self.dev, self.obs_scaler.mean.float(), self.obs_scaler.var.float(), self.obs_scaler.eps, self.obs_scaler.clip)
                self._packed.copy_(self.model._packed); self._log_std.copy_(self.model.log_std_parameter.detach())
            ro.obs[0].copy_(obs_raw)
            ro.run(self._ro_mode)
            v = self.val_scaler(ro.values.reshape(-1, 1), inverse=True).reshape(self.T + 1, self.N)
            self.b_val, self.b_done = v[:self.T], ro.dones.float()
            return ro.obs[self.T], v[self.T], self.env._task.extras_dict(ro.extras[self.T - 1])
        for t in range(self.T):
            mean, log_std, value = self._policy(obs_raw)
            act = mean + log_std.exp() * torch.randn_like(mean)
            o, rew, done, extras = self.env.step(act)
            self.b_obs[t], self.b_act[t], self.b_logp[t] = obs_raw, act, self._logp(mean, log_std, act)
            self.b_val[t], self.b_rew[t], self.b_done[t] = value, rew, done.float()
            obs_raw = o["obs"]
        _, _, last_value = self._policy(obs_raw)
        return obs_raw, last_value, extras

    def _mark(self, phase):
        """Timing hook (tools/bench_ppo_update.py): with self.phase_marks a list, a device event is recorded at each phase boundary of update()."""
        if self.phase_marks is not None:
            ev = torch.cuda.Event(enable_timing=True); ev.record(); self.phase_marks.append((phase, ev))

    def _check_pack_status(self, status: int):
        if status:
            from ..policies.prepare import pack_status_error
            self._pstatus.zero_()
            raise pack_status_error(int(status), self._kind)

    def _prepare_batch(self, ret, adv):
        """hip_prepare: lm_ppo_batch_stats + lm_ppo_batch_apply on the rollout's buffers (three launches): both scalers are merged in their state
        blocks, and the normalised batch is written into buffers kept per batch size."""
        from ..policies.prepare import batch_apply, batch_stats, batch_stats_workspace
        obs = self.b_obs.reshape(-1, self.n_obs); ret, adv, old_val = ret.reshape(-1), adv.reshape(-1), self.b_val.reshape(-1)
        B = obs.shape[0]
        if B not in self._prep:
            z = lambda *s: torch.empty(*s, device=self.dev, dtype=torch.float32)
            self._prep[B] = (batch_stats_workspace(B, self.n_obs, self.dev), (z(B, self.n_obs), z(B), z(B), z(B)))
        ws, out = self._prep[B]
        batch_stats(obs, ret, adv, self._sums, ws)
        batch_apply(obs, ret, old_val, adv, self._sums, self.obs_scaler.state, self.val_scaler.state, self.freeze_obs_scaler, self.obs_scaler.eps,
                    self.obs_scaler.clip, out)
        return obs, ret, old_val, out

    def update(self, last_value, fetch: bool = True):
        """One PPO update on the rollout collect() has just filled.  Returns the statistics of the last mini-batch {kl, loss_pi, loss_v, lr}.
        fetch=False (hip_prepare and hip_optimizer together only) returns None instead: the statistics, the optimiser state and the pack status stay
        on the device, nothing is copied to the host and nothing waits for the device; self.lr and opt.param_groups are refreshed by the next
        update that fetches, which is also where a bad weight seen by the pack kernel is reported."""
        if not fetch and not (self.hip_prepare and self.hip_optimizer):
            raise ValueError("update(fetch=False) leaves the statistics on the device: it needs hip_prepare=True and hip_optimizer=True")
        self._mark("start")
        if self._fused_update:      # one launch over the plan's own buffers (int64 dones), bit for bit compute_gae
            from ..policies.mlp_model import gae
            dones = self.rollout.dones if self.rollout is not None else self.b_done.long()
            ret, adv = gae(self.b_rew, self.b_val, dones, last_value, self.gamma, self.lam)
        else:
            ret, adv = D.compute_gae(self.b_rew, self.b_val, self.b_done, last_value, self.gamma, self.lam)
        self._mark("gae")
        act, old_logp = self.b_act.reshape(-1, 12), self.b_logp.reshape(-1)
        if self.hip_prepare:      # scalers, global advantage normalisation and the normalised batch: three launches, no torch
            obs, ret, old_val, (obs_n, ret_n, old_val_n, adv) = self._prepare_batch(ret, adv)
        else:
            g_ret, g_adv = D.all_gather_rollout(ret, adv)                 # RCCL all-gather over xGMI when world > 1
            adv = (adv - g_adv.mean()) / (g_adv.std() + 1e-8)             # global advantage normalisation
            obs, old_val = self.b_obs.reshape(-1, self.n_obs), self.b_val.reshape(-1)
            ret, adv = ret.reshape(-1), adv.reshape(-1)
            if not self.freeze_obs_scaler: self.obs_scaler.update(obs)
            self.val_scaler.update(ret.unsqueeze(-1))      # preprocessors train on the first epoch's data
            obs_n = self.obs_scaler(obs); ret_n = self.val_scaler(ret.unsqueeze(-1)).squeeze(-1); old_val_n = self.val_scaler(old_val.unsqueeze(-1)).squeeze(-1)
        n = obs.shape[0]; stats = {}
        # what the mini-batches below are cut from (references, no copies): read by the tests of the HIP update
        self.last_batch = {"obs_n": obs_n, "act": act, "old_logp": old_logp, "old_val_n": old_val_n, "adv": adv, "ret_n": ret_n, "ret": ret}
        self._mark("normalise")
        if self.hip_optimizer:
            from ..policies.optim import STATE
            self._run_epochs(obs_n, act, old_logp, old_val_n, adv, ret_n)
            self._mark("epochs")
            if not fetch:
                return None
            h = self._fetch.cpu()                                                  # the update's one device-to-host copy
            ns = self._ostate.numel()
            if self.hip_prepare: self._check_pack_status(int(h[ns + 2:].view(torch.int32)[0]))
            self.lr = float(h[STATE["lr"]])
            for gp in self.opt.param_groups: gp["lr"] = self.lr
            return {"kl": float(h[STATE["kl"]]), "loss_pi": float(h[ns]), "loss_v": float(h[ns + 1]), "lr": self.lr}
        for epoch in range(self.epochs):
            perm = torch.randperm(n, device=self.dev) if self.mb > 1 else None
            kls = []
            for i in range(self.mb):
                idx = slice(None) if perm is None else perm[i * n // self.mb:(i + 1) * n // self.mb]
                if self._fused_update:
                    # loss and gradient of the mini-batch in one fused launch (+ its reduction) straight into the flat .grad buffer; a permuted
                    # mini-batch is gathered with torch and handed over contiguous
                    self._hip_grad(*(t[idx] for t in (obs_n, act, old_logp, old_val_n, adv, ret_n)))
                    st = self._ppo_stats.clone(); loss_pi, loss_v = st[0], st[1]; kls.append(st[2])
                    if self.world > 1:
                        dist.all_reduce(self._gflat); self._gflat /= self.world
                else:
                    loss, loss_pi, loss_v, kl_mb, _ = ppo_loss(self.model(obs_n[idx]), act[idx], old_logp[idx], old_val_n[idx], adv[idx], ret_n[idx],
                                                               self.rclip, self.vclip, self.vscale, self.escale)
                    kls.append(kl_mb)
                    self.opt.zero_grad(set_to_none=True); loss.backward()
                    if self.world > 1:
                        flat = torch.cat([p.grad.reshape(-1) for p in self.model.parameters() if p.grad is not None])
                        dist.all_reduce(flat); flat /= self.world; o = 0
                        for p in self.model.parameters():
                            if p.grad is not None:
                                p.grad.copy_(flat[o:o + p.numel()].view_as(p)); o += p.numel()
                torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.gclip)
                self.opt.step()
                if self.min_log_std is not None:
                    with torch.no_grad(): self.model.log_std_parameter.clamp_(min=self.min_log_std)
            kl = torch.stack(kls).mean()
            if self.world > 1:
                dist.all_reduce(kl); kl /= self.world
            kl = float(kl)                                                        # KLAdaptiveRL (skrl): lr /= 1.5 above 2*thr, *= 1.5 below thr/2
            if self.kl_thr > 0:                                                   # kl_threshold 0 = fixed learning rate
                if kl > self.kl_thr * 2: self.lr = max(self.lr / 1.5, 1e-6)
                elif kl < self.kl_thr / 2: self.lr = min(self.lr * 1.5, self.max_lr)
            for gp in self.opt.param_groups: gp["lr"] = self.lr
            stats = {"kl": kl, "loss_pi": float(loss_pi), "loss_v": float(loss_v), "lr": self.lr}
        self._mark("epochs")
        if self.hip_prepare: self._check_pack_status(int(self._pstatus.cpu()[0]))
        return stats

    def _run_epochs(self, obs_n, act, old_logp, old_val_n, adv, ret_n):
        """The epoch loop of hip_optimizer=True: per mini-batch the fused gradient launch and lm_adam_clip_step, per epoch lm_kl_adaptive_lr on
        that epoch's KL values.  Nothing in here waits for the device: the statistics of every mini-batch stay in self._stats_all, the KL
        values of epoch e in self.last_kls[e], and the state block plus the last loss_pi / loss_v are left in self._fetch for update()'s
        one copy to the host."""
        from ..policies.optim import adam_clip_step, kl_adaptive_lr
        n, E, mb = obs_n.shape[0], self.epochs, self.mb
        if self._stats_all is None or self._stats_all.shape[0] != E * mb:
            self._stats_all = torch.zeros(E * mb, 4, device=self.dev)
            self.last_kls = self._stats_all[:, 2].unflatten(0, (E, mb))               # a view: (epoch, mini-batch)
        b1, b2 = self.opt.defaults["betas"]; eps = self.opt.defaults["eps"]
        clamp = None if self.min_log_std is None else (self._offsets["log_std_parameter"][0], 12, self.min_log_std)
        for epoch in range(E):
            perm = torch.randperm(n, device=self.dev) if mb > 1 else None
            for i in range(mb):
                idx = slice(None) if perm is None else perm[i * n // mb:(i + 1) * n // mb]
                self._hip_grad(*(t[idx] for t in (obs_n, act, old_logp, old_val_n, adv, ret_n)), stats=self._stats_all[epoch * mb + i])
                if self.world > 1:
                    dist.all_reduce(self._gflat); self._gflat /= self.world
                adam_clip_step(self._flat, self._gflat, self._m, self._v, self._ostate, b1, b2, eps, self.gclip, clamp)
            kls = self.last_kls[epoch]
            if mb > 1 or self.world > 1:
                kls = kls.contiguous()                                                 # one value is its own contiguous row
                if self.world > 1:
                    dist.all_reduce(kls); kls /= self.world
                    self.last_kls[epoch].copy_(kls)
            kl_adaptive_lr(self._ostate, kls, self.kl_thr, 1e-6, self.max_lr)
        ns = self._ostate.numel()
        self._fetch[:ns].copy_(self._ostate); self._fetch[ns:ns + 2].copy_(self._stats_all[-1, :2])

    def _hip_grad(self, obs_n, act, old_logp, old_val_n, adv, ret_n, stats=None):
        """lm_mlp_ppo_grad / lm_gnn_ppo_grad on one mini-batch: fills the flat gradient buffer (the parameters' .grad views) and `stats`
        (self._ppo_stats when not given)."""
        B = int(obs_n.shape[0]); stats = self._ppo_stats if stats is None else stats
        if self.gnn_hip_update:
            from ..policies.graph_model import gnn_ppo_grad, gnn_ppo_grad_workspace
            if B not in self._ws:
                self._ws[B] = gnn_ppo_grad_workspace(B, self.dev)
            gnn_ppo_grad(self._flat, obs_n, act, old_logp, old_val_n, adv, ret_n, self.rclip, self.vclip, self.vscale, self.escale,
                         grad=self._gflat, stats=stats, workspace=self._ws[B])
            return
        from ..policies.mlp_model import mlp_ppo_grad, ppo_grad_workspace
        if B not in self._ws:
            self._ws[B] = ppo_grad_workspace(self.n_obs, B, self.dev)
        mlp_ppo_grad(self._flat, obs_n, act, old_logp, old_val_n, adv, ret_n, self.rclip, self.vclip, self.vscale, self.escale,
                     grad=self._gflat, stats=stats, workspace=self._ws[B])

    # ------------------------------------------------------------------ checkpoints (what the reference's agents write as best_agent.pt: policy,
    # value head, optimiser and both preprocessors; tools/eval_policy.py and train/evaluate.py read them back)
    def _moments_to_opt(self):
        """hip_optimizer: self.opt's state as torch.optim.Adam would hold it after the steps taken so far (copies of the flat blocks)."""
        from ..policies.optim import STATE
        step = float(self._ostate[STATE["step"]])
        self.opt.state.clear()
        if step > 0:
            for name, p in self.model.named_parameters():
                o, shape = self._offsets[name]
                self.opt.state[p] = {"step": torch.tensor(step, dtype=torch.float32), "exp_avg": self._m[o:o + p.numel()].view(shape).clone(),
                                     "exp_avg_sq": self._v[o:o + p.numel()].view(shape).clone()}

    def _moments_from_opt(self):
        """hip_optimizer: the flat blocks and the state block from what self.opt has just loaded (a parameter without state: zeros)."""
        from ..policies.optim import optim_state
        self._m.zero_(); self._v.zero_(); step = 0.0
        for name, p in self.model.named_parameters():
            st = self.opt.state.get(p)
            if st:
                o, _ = self._offsets[name]
                self._m[o:o + p.numel()].copy_(st["exp_avg"].reshape(-1)); self._v[o:o + p.numel()].copy_(st["exp_avg_sq"].reshape(-1))
                step = float(st["step"])
        optim_state(self.dev, self.lr, step, state=self._ostate)
        self.opt.state.clear()

    def state_dict(self):
        if self.hip_prepare and self.hip_optimizer:      # updates with fetch=False leave the rate on the device: one copy brings it and the pack status
            from ..policies.optim import STATE
            h = self._fetch.cpu()
            self._check_pack_status(int(h[self._ostate.numel() + 2:].view(torch.int32)[0]))
            self.lr = float(h[STATE["lr"]])
            for gp in self.opt.param_groups: gp["lr"] = self.lr
        elif self.hip_prepare:      # a checkpoint of weights the pack kernel has flagged is refused like an update's fetch
            self._check_pack_status(int(self._pstatus.cpu()[0]))
        if self.hip_optimizer:      # the checkpoint is torch.optim.Adam's in every mode
            self._moments_to_opt()
            try:
                return self._state_dict()
            finally:
                self.opt.state.clear()
        return self._state_dict()

    def _state_dict(self):
        return {"model":{k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}, "model_class": type(self.model).__name__,
                "num_observations": self.n_obs, "obs_scaler": self.obs_scaler.state_dict(), "val_scaler": self.val_scaler.state_dict(),
                "lr": float(self.lr), "optimizer": self.opt.state_dict()}

    def load_state_dict(self, sd):
        assert int(sd["num_observations"]) == self.n_obs, (sd["num_observations"], self.n_obs)
        self.model.load_state_dict(sd["model"])
        self.obs_scaler.load_state_dict(sd["obs_scaler"]); self.val_scaler.load_state_dict(sd["val_scaler"])
        self.opt.load_state_dict(sd["optimizer"])
        self.lr = float(sd["lr"])
        for gp in self.opt.param_groups: gp["lr"] = self.lr
        if self.hip_optimizer:
            self._moments_from_opt()
            if self.hip_prepare: self._fetch[:self._ostate.numel()].copy_(self._ostate)      # the fetch block mirrors the state block between updates

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, map_location="cpu", weights_only=False))

    def train(self, timesteps: int, log_every: int = 10, log=print):
        obs = self.env.reset()["obs"]; history = []; t0 = time.perf_counter()
        for it in range(timesteps // self.T):
            obs, last_value, extras = self.collect(obs)
            logged = it % log_every == 0 or it == timesteps // self.T - 1
            st = self.update(last_value, fetch=logged) if (self.hip_prepare and self.hip_optimizer) else self.update(last_value)
            if logged:
                ex = D.global_extras(extras, self.N)
                rec = {"iteration": it, "timesteps": (it + 1) * self.T, "wall_s": time.perf_counter() - t0, "mean_reward": float(self.b_rew.mean()),
                       "success_rate": float(ex["env/success_rate"]), "std": float(self.model.log_std_parameter.exp().mean()), **st}
                history.append(rec); log(rec)
        return history
