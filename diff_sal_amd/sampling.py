"""Sampling loops of the DiffSal trainer, re-built around a non-mutating denoiser.

Call-surface parity:
  * ``DiffusionSampler`` carries the schedule constants of ``DiffusionTrainer.__init__``
    (R/diffusion_trainer.py:47-76) and its sampling methods ``q_sample`` (:122), ``predict_noise_from_start``
    (:434), ``sample_ddim`` (:440-480), ``sample_image`` (:546-640);
  * ``generalized_steps`` keeps the signature of the legacy helper R/util/denoising.py:9-33.

Differences, on purpose: no ``copy.deepcopy`` of the feature list per step (the denoiser does not mutate
it, D4); the DPM-Solver branch actually runs (D1), wraps the x0-predicting net as ``model_type="x_start"``
(D2) and forwards the audio conditioning (D3); alpha-bar look-ups are host scalars, so a sampling loop has
no device->host synchronisation.
"""
from __future__ import annotations

import contextlib
from typing import Optional, Sequence

import torch

from .diffusion_utils import get_beta_schedule, to_torch
from .dpm_solver import DPM_Solver, NoiseScheduleVP, _lincomb, model_wrapper

Tensor = torch.Tensor


class DiffusionSampler:
    def __init__(self, model, *, beta_schedule="cosine", beta_start=1e-4, beta_end=0.02,
                 num_diffusion_timesteps=1000, training_target="x0", sample_type="ddim", timesteps=1, eta=0.0,
                 skip_type="logSNR", dpm_solver_order=2, dpm_solver_method="multistep", dpm_solver_type="dpmsolver",
                 lower_order_final=False, denoise=True, thresholding=False, device=None, hip_graph="auto",
                 step_invariant_shortcut=False, fused_update=True, noise_source="torch", seed=0, clip_passes=None):
        """``model`` exposes ``decoder_net`` and optionally ``visual_net`` / ``audio_net`` / ``forward_vggish``
        (a ``VideoSaliencyModel``; a DDP/DataParallel wrapper is unwrapped through ``.module``).
        Keyword names = the YAML fields the trainer reads (R/cfgs/diffusion.yml:24-28, 37, 63-78)."""
        assert training_target in ("x0", "noise")
        if noise_source not in ("torch", "device"):
            raise ValueError(f"unknown noise_source {noise_source!r}; choose 'torch' or 'device'")
        self.model = getattr(model, "module", model)
        self.training_target = training_target
        self.sample_type, self.timesteps, self.eta = sample_type, int(timesteps), float(eta)
        self.skip_type, self.dpm_solver_order = skip_type, int(dpm_solver_order)
        self.dpm_solver_method, self.dpm_solver_type = dpm_solver_method, dpm_solver_type
        self.lower_order_final, self.denoise, self.thresholding = bool(lower_order_final), bool(denoise), bool(thresholding)
        betas = to_torch(get_beta_schedule(beta_schedule, beta_start=beta_start, beta_end=beta_end,
                                           num_diffusion_timesteps=num_diffusion_timesteps))
        alphas_hat = (1.0 - betas).cumprod(dim=0)  # host tables; same fp32 arithmetic as the trainer
        self.betas = betas
        self.alphas_hat = alphas_hat
        self.alphas_hat_prev = torch.cat([torch.ones(1), alphas_hat[:-1]], dim=0)
        self.sqrt_alphas_hat = torch.sqrt(alphas_hat)
        self.sqrt_one_minus_alphas_hat = torch.sqrt(1.0 - alphas_hat)
        self.sqrt_recip_alphas_hat = torch.sqrt(1.0 / alphas_hat)
        self.sqrt_recipm1_alphas_hat = torch.sqrt(1.0 / alphas_hat - 1)
        self.log_one_minus_alphas_hat = torch.log(1.0 - alphas_hat)
        # DDPM posterior tables exactly as the trainer builds them (R/diffusion_trainer.py:66-75), including its
        # coefficient quirk: coef1 uses sqrt(alphas_hat[t]) where the DDPM paper has sqrt(alphas_hat[t-1])
        self.posterior_variance = betas * (1.0 - self.alphas_hat_prev) / (1.0 - alphas_hat)
        self.posterior_log_variance_clipped = torch.log(torch.maximum(self.posterior_variance, torch.tensor(1e-20)))
        self.posterior_mean_coef1 = betas * torch.sqrt(alphas_hat) / (1.0 - alphas_hat)
        self.posterior_mean_coef2 = (1.0 - self.alphas_hat_prev) * torch.sqrt(1.0 - betas) / (1.0 - alphas_hat)
        self.num_timesteps = betas.shape[0]
        self.device = device
        # Optional modes, both OFF by default and reported separately from the headline metric:
        #  hip_graph: capture one whole sampling trajectory per input shape in a HIP graph and replay it
        #    (the loop is enqueue-only, so it is capturable); removes host launch cost at small batch.
        #  step_invariant_shortcut: in visual-only eval mode the denoiser output does not depend on (x, t)
        #    (the noise map is frame 8 of 9, ReduceTemp reads frames 0-4), so every step of a
        #    trajectory returns the same x0 and the sample equals ONE network evaluation.
        #    "auto" (the default): replay for batches of at most `graph_batch_max` clips -- one or two clips per step are bound
        #    by the host's ~20 us per launch, not by the kernels (B = 1: 1.9 ms eager vs 1.1-1.4 ms replayed); larger batches
        #    run eagerly (the loop is GPU-bound there).  True / False force it.
        self.hip_graph = hip_graph if hip_graph == "auto" else bool(hip_graph)
        self.graph_batch_max = 2
        self.step_invariant_shortcut = bool(step_invariant_shortcut)
        #  fused_update (ON by default: same arithmetic, bit-equal results): the DPM-Solver branch folds each step's final
        #    resize + x0->noise conversion + multistep update into the denoiser's last kernel (SalUNet.forward_fused_update).
        self.fused_update = bool(fused_update)
        #  noise_source: "torch" (the default) draws x_T and the per-step noise of DDIM with eta > 0 / DDPM from torch's stateful
        #    generator, as the reference does.  "device": a counter-based generator (Philox4x32-10, include/diffsal.h) keyed by
        #    ``seed`` and counted by (clip id, draw, element): a clip's prediction no longer depends on the batch it sits in, its
        #    position there or the number of ranks of a sweep; the step noise is generated inside the fused step tail, and a
        #    stochastic trajectory can be replayed from a graph (ids and seed are device buffers rewritten before a replay).
        #  clip_passes (None: on with "device", off with "torch"): the denoiser evaluates a batch one clip per pass
        #    (SalUNet.max_clips_per_pass = 1 for the trajectory).  Its kernels choose tiles by the batch size, so a clip's output moves
        #    by ~1e-6 with the batch it is evaluated in; one clip per pass makes the whole prediction, not only the noise, bit-equal
        #    on any layout, at the price of the batched launches (B = 1 is unaffected).  False keeps the batched passes: the noise
        #    is still layout-independent, the prediction then agrees across layouts to ~1e-6.  sample_image applies the same rule
        #    to the encoders it runs in front of the trajectory.
        self.noise_source, self.seed = noise_source, int(seed)
        self.clip_passes = (noise_source == "device") if clip_passes is None else bool(clip_passes)
        if self.step_invariant_shortcut:
            self._check_shortcut_precondition()
        self._graphs = {}

    def _check_shortcut_precondition(self) -> None:
        """The F1 shortcut is only valid when the denoiser output provably ignores (x, t) in visual-only eval mode: the
        noise map must be a frame the temporal reduction never reads, and the network must predict x0 directly."""
        net = self.model.decoder_net
        if self.training_target != "x0":
            raise ValueError("step_invariant_shortcut needs training_target='x0' (a noise-predicting net is converted with "
                             "x_t, so the sample depends on every step)")
        tl = getattr(net, "temporal_list", None)
        if tl is None or not getattr(net, "image_based", False):
            raise ValueError("step_invariant_shortcut needs a SalUNet with image_based=True (the noise map is appended as "
                             "the LAST frame; otherwise it is not known to be outside the ReduceTemp window)")
        # frames are [8 visual..., noise]; ReduceTemp(kernel = stride = kt) reads frames 0 .. kt-1 only
        frames_in = 8 + 1
        if any(int(kt) >= frames_in for kt in tl):
            raise ValueError(f"step_invariant_shortcut: temporal_list={list(tl)} reaches the noise frame (index {frames_in - 1}); "
                             "the output then depends on (x, t)")

    # ---- forward process (training side, K16) ----
    def q_sample(self, x_start: Tensor, t: int, noise: Optional[Tensor] = None) -> Tensor:
        if noise is None:
            noise = torch.randn_like(x_start)
        return _lincomb(x_start, self.sqrt_alphas_hat[t], noise, self.sqrt_one_minus_alphas_hat[t])

    def predict_noise_from_start(self, x_t: Tensor, t: int, x0: Tensor) -> Tensor:
        r, rm1 = float(self.sqrt_recip_alphas_hat[t]), float(self.sqrt_recipm1_alphas_hat[t])
        return _lincomb(x_t, r / rm1, x0, -1.0 / rm1)

    # ---- DDPM ancestral sampling (R/diffusion_trainer.py:482-527; the caller at :574-580 is broken upstream) ----
    def predict_start_from_noise(self, x_t: Tensor, t: int, noise: Tensor) -> Tensor:
        return _lincomb(x_t, float(self.sqrt_recip_alphas_hat[t]), noise, -float(self.sqrt_recipm1_alphas_hat[t]))

    def q_posterior(self, x_start: Tensor, x_t: Tensor, t: int):
        mean = _lincomb(x_start, float(self.posterior_mean_coef1[t]), x_t, float(self.posterior_mean_coef2[t]))
        return mean, self.posterior_variance[t], self.posterior_log_variance_clipped[t]

    @torch.no_grad()
    def p_mean_variance(self, x: Tensor, t: int, img, clip_denoised: bool = True, audio_cond: Optional[Tensor] = None):
        """``clip_denoised`` is accepted and, as in the reference (:505-506: ``x_recon.clamp(-1, 1)`` without assignment),
        has no effect."""
        net = self.model.decoder_net
        t_tensor = torch.full((x.shape[0],), t, dtype=torch.int64, device=x.device)
        out = net(x, t_tensor, img, audio_cond) if audio_cond is not None else net(x, t_tensor, img)
        x_recon = out if self.training_target == "x0" else self.predict_start_from_noise(x, t, out)
        return self.q_posterior(x_recon, x, t)

    # ---- device noise (noise_source="device") ----
    def _noise_device(self, like=None):
        dev = like.device if like is not None else torch.device(self.device if self.device is not None else "cuda")
        if torch.device(dev).type != "cuda":
            raise RuntimeError("diff_sal_amd device noise runs on the GPU only (no CPU fallback); got a CPU tensor")
        return dev

    def _noise_key(self, clip_ids, x):
        """(ids, seed) device buffers of a trajectory, or None with noise_source="torch" / without clip ids."""
        if self.noise_source != "device":
            if clip_ids is not None:
                raise ValueError("clip_ids are only used with noise_source='device'")
            return None
        dev = self._noise_device(x)
        if clip_ids is None:
            return None
        from . import ops
        ids, seed = ops.noise_key(clip_ids, self.seed, dev)
        if ids.numel() != x.shape[0]:
            raise ValueError(f"{ids.numel()} clip ids for {x.shape[0]} clips")
        return ids, seed

    def _step_noise(self, x, key, draw):
        """N(0, 1) of the shape of ``x`` for step noise number ``draw``: torch's generator, or the device generator."""
        if self.noise_source != "device":
            return torch.randn_like(x)
        if key is None:
            raise ValueError("noise_source='device': a stochastic trajectory needs clip_ids")
        from . import ops
        return ops.philox_normal(key[0], key[1], draw, tuple(x.shape[1:]))

    @contextlib.contextmanager
    def _passes(self):
        """One clip per denoiser pass for the duration of a trajectory when ``clip_passes`` is on (see __init__)."""
        net = self.model.decoder_net
        if not self.clip_passes or not hasattr(net, "max_clips_per_pass"):
            yield
            return
        own = net.__dict__.get("max_clips_per_pass")
        net.max_clips_per_pass = 1
        try:
            yield
        finally:
            if own is None:
                del net.max_clips_per_pass          # back to the class default
            else:
                net.max_clips_per_pass = own

    def _state_shape(self, n):
        h, w = self.model.decoder_net.img_size
        return (int(n), 1, int(h), int(w))

    def initial_noise(self, clip_ids, shape=None, device=None) -> Tensor:
        """x_T of the clips ``clip_ids`` (draw 0 of the device generator): [len(clip_ids), *shape[1:]] fp32.  ``shape`` is the
        shape of the whole batch, as in ``torch.randn(shape)`` (default: [N, 1, *decoder_net.img_size])."""
        if self.noise_source != "device":
            raise ValueError("initial_noise needs noise_source='device' (torch noise: the caller draws x_T)")
        from . import ops
        dev = clip_ids.device if isinstance(clip_ids, Tensor) and clip_ids.is_cuda else (device if device is not None else self._noise_device())
        ids, seed = ops.noise_key(clip_ids, self.seed, dev)
        shape = self._state_shape(ids.numel()) if shape is None else tuple(int(v) for v in shape)
        if shape[0] != ids.numel():
            raise ValueError(f"{ids.numel()} clip ids for a batch of shape {shape}")
        return ops.philox_normal(ids, seed, 0, shape[1:])

    def _start(self, x, clip_ids, img):
        """(x, key) at the start of a trajectory: x_T from the device generator when the caller passed x=None."""
        if self.noise_source == "device" and x is not None and not x.is_cuda:
            raise RuntimeError("diff_sal_amd device noise runs on the GPU only (no CPU fallback); got a CPU tensor")
        if x is None:
            if self.noise_source != "device" or clip_ids is None:
                raise ValueError("x=None needs noise_source='device' and clip_ids")
            dev = img[0].device if img else None
            x = self.initial_noise(clip_ids, device=dev)
        return x, self._noise_key(clip_ids, x)

    @torch.no_grad()
    def p_sample(self, x: Tensor, t: int, img, clip_denoised: bool = True, audio_cond: Optional[Tensor] = None,
                 noise: Optional[Tensor] = None, noise_key=None) -> Tensor:
        """``noise_key = (ids, seed, draw)`` (noise_source="device"): the step noise comes from the device generator, inside
        the denoiser's last kernel where the fused tail applies."""
        if noise is None and noise_key is not None and self._tail_fusable(x):
            net = self.model.decoder_net
            t_tensor = torch.full((x.shape[0],), t, dtype=torch.int64, device=x.device)
            cz = 0.0 if t == 0 else float(torch.exp(0.5 * self.posterior_log_variance_clipped[t]))
            _, xn = net.forward_fused_update(x, t_tensor, img, audio_cond, ex=0.0, e0=1.0, A=float(self.posterior_mean_coef2[t]),
                                             c0=0.0, b0=float(self.posterior_mean_coef1[t]), cz=cz,
                                             noise_key=noise_key if cz != 0.0 else None)
            return xn
        mean, _, log_var = self.p_mean_variance(x, t, img, clip_denoised=clip_denoised, audio_cond=audio_cond)
        if t == 0:
            return mean                                   # no noise at the last step (:517-519)
        if noise is None:
            noise = torch.randn_like(x) if noise_key is None else self._step_noise(x, noise_key[:2], noise_key[2])
        return _lincomb(mean, 1.0, noise, float(torch.exp(0.5 * log_var)))

    @torch.no_grad()
    def sample_ddpm(self, x: Optional[Tensor], img=None, audio_cond: Optional[Tensor] = None, noises=None, clip_ids=None) -> Tensor:
        """``timesteps`` ancestral steps on the grid ``range(0, T, T // timesteps)`` reversed (:574-578).  The conditioning
        list is never mutated here, so the reference's per-step ``copy.deepcopy`` is not needed.
        noise_source="device": ``clip_ids`` (one int64 per row) name the clips; ``x=None`` starts from their x_T."""
        x, key = self._start(x, clip_ids, img)
        if noises is None and self.noise_source == "device" and key is None:
            raise ValueError("noise_source='device': a stochastic trajectory needs clip_ids")
        with self._passes():
            # torch noise stays eager (a seeded run draws the numbers the eager loop draws); device noise replays like DDIM
            if noises is None and key is not None and self._use_graph(x, device_noise=True):
                return self._graphed(self._sample_ddpm, x, img, audio_cond, key)
            return self._sample_ddpm(x, img, audio_cond, key, noises)

    def _sample_ddpm(self, x, img, audio_cond, key=None, noises=None):
        skip = self.num_timesteps // self.timesteps
        seq = list(range(0, self.num_timesteps, skip))
        for i, t in enumerate(reversed(seq)):
            nk = None if key is None or noises is not None else (key[0], key[1], i + 1)
            x = self.p_sample(x, t, img, audio_cond=audio_cond, noise=None if noises is None else noises[i], noise_key=nk)
        return x

    def _tail_fusable(self, x) -> bool:
        """The fused DDIM / DDPM step tail applies when the denoiser is ours in eval mode and predicts x0."""
        net = self.model.decoder_net
        return (self.fused_update and hasattr(net, "forward_fused_update") and not getattr(net, "training", False)
                and x.is_cuda and self.training_target == "x0")

    # ---- DDIM (the reference's live sampler) ----
    def _shortcut(self, x, img, audio_cond):
        net = self.model.decoder_net
        t = torch.full((x.size(0),), self.num_timesteps - 1, dtype=torch.int64, device=x.device)
        return net(x, t, img, None)

    def _use_graph(self, x, device_noise: bool = False) -> bool:
        if not x.is_cuda or torch.cuda.is_current_stream_capturing():
            return False
        if self.hip_graph == "auto":
            net = self.model.decoder_net
            from . import ops
            # only our own denoiser in eval mode is known to be capturable (no host sync, no allocation outside the pool); a
            # stochastic trajectory (DDIM with eta > 0) on torch's generator stays eager so that a seeded run draws the numbers
            # the eager loop draws -- device noise has no state to advance and is replayed like a deterministic trajectory;
            # per-launch profiling events cannot be recorded inside a capture
            if ops.PROFILE is not None or (self.sample_type != "dpmsolver" and self.eta != 0.0 and not device_noise):
                return False
            return x.size(0) <= self.graph_batch_max and hasattr(net, "forward_fused_update") and not getattr(net, "training", False)
        return bool(self.hip_graph)

    def _graph_state(self):
        """Everything a captured trajectory bakes in besides the input shapes: the decoder's kernel-layout weights (their
        device pointers change when parameters are updated, re-loaded or the precision mode changes) and the sampler's
        own hyper-parameters (they decide the time grid and every coefficient)."""
        net = self.model.decoder_net
        epoch = net.pack_epoch() if hasattr(net, "pack_epoch") else None
        return (epoch, bool(getattr(net, "training", False)), self.sample_type, self.timesteps, self.eta, self.skip_type,
                self.dpm_solver_order, self.dpm_solver_method, self.dpm_solver_type, self.lower_order_final, self.denoise,
                self.thresholding, self.training_target, self.fused_update, self.clip_passes, self.noise_source)

    def _graphed(self, fn, x, img, audio_cond, noise_key=None):
        """Replay (capturing on first use) ``fn(x, img, audio_cond)`` as one HIP graph per input signature; a graph is
        re-captured when the decoder's packed weights or the sampler's hyper-parameters changed since its capture.
        ``noise_key`` (ids, seed): device noise; the two buffers are static inputs like x, so other clips or another seed
        replay the same capture."""
        key = (fn.__name__, tuple(x.shape), tuple(tuple(f.shape) for f in img), None if audio_cond is None else tuple(audio_cond.shape),
               noise_key is not None)
        call = fn if noise_key is None else (lambda a, b, c: fn(a, b, c, sk))
        state = self._graph_state()
        ent = self._graphs.get(key)
        if ent is not None and ent[0] != state:
            ent = None              # stale: drop it (frees its private pool) and capture again
            del self._graphs[key]
        if ent is not None and ent[1] is None:
            return fn(x, img, audio_cond) if noise_key is None else fn(x, img, audio_cond, noise_key)   # failed to capture once: eager
        if ent is None:
            sx, simg = x.clone(), [f.clone() for f in img]
            sa = None if audio_cond is None else audio_cond.clone()
            sk = None if noise_key is None else tuple(t.clone() for t in noise_key)
            # the warm-up (library load, weight packing, allocator pools) must not move the caller's random stream
            dev = x.device
            rng_cpu, rng_dev = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
            try:
                call(sx, simg, sa)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                # thread_local: a HIP call from another thread of the process (pin-memory thread, collective watchdog) must
                # not invalidate this capture
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    out = call(sx, simg, sa)
            except Exception as e:  # noqa: BLE001 -- any capture failure: remember it, run the loop eagerly
                if self.hip_graph != "auto":
                    raise
                import warnings
                warnings.warn(f"diff_sal_amd: HIP-graph capture of {fn.__name__} failed ({type(e).__name__}: {e}); "
                              "this input signature runs eagerly from now on")
                torch.cuda.synchronize()
                self._graphs[key] = (state, None, None, None, None, None, None)
                torch.set_rng_state(rng_cpu)
                torch.cuda.set_rng_state(rng_dev, dev)
                return fn(x, img, audio_cond) if noise_key is None else fn(x, img, audio_cond, noise_key)
            torch.set_rng_state(rng_cpu)
            torch.cuda.set_rng_state(rng_dev, dev)
            ent = (state, g, sx, simg, sa, out, sk)
            self._graphs[key] = ent
        _, g, sx, simg, sa, out, sk = ent
        sx.copy_(x)
        for d, s_ in zip(simg, img):
            d.copy_(s_)
        if sa is not None:
            sa.copy_(audio_cond)
        if sk is not None:
            for d, s_ in zip(sk, noise_key):
                d.copy_(s_)
        g.replay()
        return out.clone()

    @torch.no_grad()
    def sample_ddim(self, x: Optional[Tensor], img: Optional[Sequence[Tensor]] = None, audio_cond: Optional[Tensor] = None,
                    clip_ids=None) -> Tensor:
        """noise_source="device": ``clip_ids`` (one int64 per row) name the clips; ``x=None`` starts from their x_T."""
        x, key = self._start(x, clip_ids, img)
        if self.step_invariant_shortcut and audio_cond is None:
            return self._shortcut(x, img, audio_cond)
        if self.eta != 0.0 and self.noise_source == "device" and key is None and self.timesteps > 1:
            raise ValueError("noise_source='device': a stochastic trajectory needs clip_ids")
        with self._passes():
            if self._use_graph(x, device_noise=key is not None):
                return self._graphed(self._sample_ddim, x, img, audio_cond, key)
            return self._sample_ddim(x, img, audio_cond, key)

    def _sample_ddim(self, x, img, audio_cond, key=None):
        skip = self.num_timesteps // self.timesteps
        seq = list(range(0, self.num_timesteps, skip))
        seq_next = [-1] + seq[:-1]
        n = x.size(0)
        net = self.model.decoder_net
        # fused tail (one forward_fused_update per step, nothing after the network): whenever the step draws nothing (eta = 0)
        # or draws from the device generator; torch noise keeps the stand-alone launches and its generator's numbers
        fused = self._tail_fusable(x) and (self.eta == 0.0 or key is not None)
        for step, (time, time_next) in enumerate(zip(reversed(seq), reversed(seq_next))):
            t_tensor = torch.full((n,), time, dtype=torch.int64, device=x.device)
            alpha = float(self.alphas_hat[time])
            if fused and time_next >= 0:
                alpha_next = float(self.alphas_hat[time_next])
                c1 = self.eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)) ** 0.5
                c2 = ((1 - alpha_next) - c1 ** 2) ** 0.5
                r, rm1 = float(self.sqrt_recip_alphas_hat[time]), float(self.sqrt_recipm1_alphas_hat[time])
                _, x = net.forward_fused_update(x, t_tensor, img, audio_cond, ex=r / rm1, e0=-1.0 / rm1, A=0.0, c0=c2,
                                                b0=float(self.sqrt_alphas_hat[time_next]), cz=c1,
                                                noise_key=None if c1 == 0.0 else (key[0], key[1], step + 1))
                continue
            out = net(x, t_tensor, img, audio_cond)
            if self.training_target == "x0":
                x_start = out
                pred_noise = None if time_next < 0 else self.predict_noise_from_start(x, time, x_start)
            else:
                pred_noise = out
                x_start = _lincomb(x, alpha ** -0.5, pred_noise, -((1 - alpha) ** 0.5) / alpha ** 0.5)
            if time_next < 0:
                x = x_start
                continue
            alpha_next = float(self.alphas_hat[time_next])
            c1 = self.eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)) ** 0.5
            c2 = ((1 - alpha_next) - c1 ** 2) ** 0.5
            if c1 != 0.0:
                x = _lincomb(x_start, float(self.sqrt_alphas_hat[time_next]), self._step_noise(x, key, step + 1), c1, pred_noise, c2)
            else:  # eta = 0 (the shipped config): deterministic, no RNG launch
                x = _lincomb(x_start, float(self.sqrt_alphas_hat[time_next]), pred_noise, c2)
        return x

    # ---- DPM-Solver (the path the reference intended, with D1-D4 fixed) ----
    @torch.no_grad()
    def sample_dpm_solver(self, x: Optional[Tensor], img=None, audio_cond: Optional[Tensor] = None, clip_ids=None) -> Tensor:
        """Deterministic: ``clip_ids`` only matter for ``x=None`` (x_T from the device generator, noise_source="device")."""
        x, _ = self._start(x, clip_ids, img)
        if self.step_invariant_shortcut and audio_cond is None:
            return self._shortcut(x, img, audio_cond)
        with self._passes():
            if self._use_graph(x):
                return self._graphed(self._sample_dpm_solver, x, img, audio_cond)
            return self._sample_dpm_solver(x, img, audio_cond)

    def _fusable(self, x) -> bool:
        """The fused step tail (SalUNet.forward_fused_update) applies when the denoiser is ours in eval mode, predicts x0,
        and the solver is the multistep noise-prediction DPM-Solver of order <= 2 without thresholding -- the shipped
        configuration (R/cfgs/diffusion.yml:63-78 with sample_type dpmsolver)."""
        net = self.model.decoder_net
        return (self.fused_update and hasattr(net, "forward_fused_update") and not net.training and x.is_cuda
                and self.training_target == "x0" and self.sample_type == "dpmsolver" and self.dpm_solver_method == "multistep"
                and self.dpm_solver_order <= 2 and not self.thresholding and self.dpm_solver_type in ("dpmsolver", "taylor"))

    def _sample_dpm_solver_fused(self, x, img, audio_cond):
        """Same trajectory as DPM_Solver.sample (dpm_solver.py), driven from its precomputed coefficient table, with every
        step's tail -- final resize, x0 -> noise conversion, multistep update -- folded into the network's last kernel:
        a denoising step is then "one SalUNet evaluation", nothing else (two elementwise launches fewer per step)."""
        net = self.model.decoder_net
        steps = self.timesteps - 1 if self.denoise else self.timesteps
        rows, last = self._fused_plan(steps)
        n = x.shape[0]
        m_prev = None
        # network times exactly as model_wrapper computes them (fp32 arithmetic on the host), as ONE device table per (plan,
        # batch, device) instead of a fill launch per step: row s is the [n] time vector of evaluation s
        tkey = (id(rows), n, str(x.device))
        t_all = self._t_tables.get(tkey) if hasattr(self, "_t_tables") else None
        if t_all is None or t_all[0] is not rows:
            vals = [r[0] for r in rows] + [last[0]]
            if torch.cuda.is_current_stream_capturing():       # no host-to-device copy inside a capture: fills instead
                tt = torch.stack([torch.full((n,), v, dtype=torch.float32, device=x.device) for v in vals])
            else:
                tt = torch.tensor(vals, dtype=torch.float32).view(-1, 1).expand(-1, n).contiguous().to(x.device)
                if not hasattr(self, "_t_tables"):
                    self._t_tables = {}
                self._t_tables[tkey] = (rows, tt)
            t_all = (rows, tt)
        t_tab = t_all[1]
        for s_, (t_net, ex, e0, A, c0, c1, two) in enumerate(rows):
            m, x = net.forward_fused_update(x, t_tab[s_], img, audio_cond, ex=ex, e0=e0, A=A, c0=c0, c1=c1,
                                            m_prev=m_prev if two else None)
            m_prev = m
        if self.denoise:                                  # denoise_to_zero_fn: data prediction at t_0 (sampler.py:542)
            t_net, alpha, sigma = last
            t_in = t_tab[len(rows)]
            noise = _lincomb(x, 1.0 / sigma, net(x, t_in, img, audio_cond), -alpha / sigma)
            x = _lincomb(x, 1.0 / alpha, noise, -sigma / alpha)
        return x

    def _fused_plan(self, steps):
        """Host scalars of every step of the fused trajectory -- network time, x0 -> noise conversion (ex, e0), update
        coefficients (A, c0, c1) -- from DPM_Solver.plan.  They depend on the sampler's hyper-parameters only, so the table is
        built once per (betas, steps, order, skip_type, ...) and reused by every trajectory (it costs ~8 ms of host time, 3 % of a
        50-step trajectory at B = 4)."""
        key = (hash(self.betas.detach().cpu().numpy().tobytes()), steps, self.dpm_solver_order, self.skip_type,
               self.lower_order_final, self.dpm_solver_type, self.sample_type, self.denoise)
        hit = self._plan_cache.get(key) if hasattr(self, "_plan_cache") else None
        if hit is not None:
            return hit
        ns = NoiseScheduleVP(schedule="discrete", betas=self.betas)
        solver = DPM_Solver(lambda *a, **k: None, ns, algorithm_type=self.sample_type)
        times, table, t_0 = solver.plan(steps, self.dpm_solver_order, self.skip_type, None, None, self.lower_order_final,
                                        self.dpm_solver_type)

        def at(tc):
            return (float((tc - 1.0 / ns.total_N) * 1000.0), float(ns.marginal_alpha(tc)), float(ns.marginal_std(tc)))

        rows = []
        for s in range(steps):
            t_net, alpha, sigma = at(times[s].reshape(1))
            A, coeffs = table[s]
            rows.append((t_net, 1.0 / sigma, -alpha / sigma, A, coeffs[0], coeffs[1] if len(coeffs) > 1 else 0.0, len(coeffs) > 1))
        plan = (rows, at(torch.ones((1,)) * t_0))
        if not hasattr(self, "_plan_cache"):
            self._plan_cache = {}
        self._plan_cache[key] = plan
        return plan

    def _sample_dpm_solver(self, x, img, audio_cond):
        if self._fusable(x):
            return self._sample_dpm_solver_fused(x, img, audio_cond)
        net = self.model.decoder_net

        def model_fn(x, t, vis_feat, **kw):
            return net(x, t, vis_feat, audio_cond)

        noise_schedule = NoiseScheduleVP(schedule="discrete", betas=self.betas)
        fn = model_wrapper(model_fn, noise_schedule,
                           model_type="x_start" if self.training_target == "x0" else "noise", guidance_type="uncond")
        solver = DPM_Solver(fn, noise_schedule, algorithm_type=self.sample_type,
                            correcting_x0_fn="dynamic_thresholding" if self.thresholding else None)
        return solver.sample(x, img, steps=self.timesteps - 1 if self.denoise else self.timesteps,
                             order=self.dpm_solver_order, skip_type=self.skip_type, method=self.dpm_solver_method,
                             lower_order_final=self.lower_order_final, denoise_to_zero=self.denoise,
                             solver_type=self.dpm_solver_type)

    @torch.no_grad()
    def sample_image(self, x: Optional[Tensor], img: Optional[Tensor] = None, audio: Optional[Tensor] = None, clip_ids=None) -> Tensor:
        """Encoders once per clip, then the per-step loop (R/diffusion_trainer.py:546-640).  noise_source="device":
        ``clip_ids`` name the clips and ``x=None`` starts from their x_T.  With ``clip_passes`` on, the encoders too evaluate a
        batch one clip per pass: their kernels choose tiles by the batch size like the denoiser's, and a feature that moves by
        ~1e-6 with the batch moves a pixel of the 8-bit export now and then."""
        m = self.model
        audio_embed = None
        if getattr(m, "audio_net", None):
            if self.clip_passes and audio is not None and audio.shape[0] > 1:
                audio_embed = torch.cat([m.forward_vggish(audio[i:i + 1])[1] for i in range(audio.shape[0])])
            else:
                _, audio_embed = m.forward_vggish(audio)
        if getattr(m, "visual_net", None):
            if self.clip_passes and img.shape[0] > 1:
                per_clip = [m.visual_net(img[i:i + 1]) for i in range(img.shape[0])]
                vis_list = [torch.cat(scale) for scale in zip(*per_clip)]
            else:
                vis_list = m.visual_net(img)
        else:  # same synthetic fall-back shapes as the reference (:564-569)
            if x is None:
                x = self.initial_noise(clip_ids)
            b, dev = x.shape[0], x.device
            vis_list = [torch.randn((b, c, 8, h, w), device=dev)
                        for c, h, w in ((768, 7, 12), (384, 14, 24), (192, 28, 48), (96, 56, 96))]
        kw = {} if clip_ids is None else {"clip_ids": clip_ids}
        if self.sample_type == "ddim":
            return self.sample_ddim(x, vis_list, audio_embed, **kw)
        if self.sample_type in ("dpmsolver", "dpmsolver++"):
            return self.sample_dpm_solver(x, vis_list, audio_embed, **kw)
        if self.sample_type == "ddpm":
            return self.sample_ddpm(x, vis_list, audio_embed, **kw)
        raise NotImplementedError(self.sample_type)


def _alpha_bar_table(b: Tensor):
    """Host list a[j] = prod_{i<j} (1 - b[i]), j = 0..len(b): a[t+1] is alpha-bar of step t and a[0] = 1 stands for
    "t = -1" (the reference builds this with a device cumprod + index_select per step, R/util/denoising.py:3-6)."""
    table = [1.0]
    for v in b.detach().double().cpu().tolist():
        table.append(table[-1] * (1.0 - v))
    return table


def compute_alpha(beta: Tensor, t: Tensor) -> Tensor:
    """alpha-bar at integer steps ``t`` (t = -1 -> 1) as a [N,1,1,1] tensor; signature of R/util/denoising.py:3."""
    table = torch.tensor(_alpha_bar_table(beta), dtype=torch.float32, device=t.device)
    return table[(t + 1).long()].view(-1, 1, 1, 1)


def _legacy_grid(seq):
    """(t, t_next) pairs of the legacy loops, last step first; t_next = -1 after the final step."""
    seq = [int(v) for v in seq]
    return list(zip(seq[::-1], ([-1] + seq[:-1])[::-1]))


def generalized_steps(x, seq, model, b, img=None, **kwargs):
    """Legacy DDIM loop, call surface of R/util/denoising.py:9-33 (dead code upstream: nothing imports it; kept because
    north_star names the ``util/denoising`` surface): ``model({"img", "input"}, t)`` predicts NOISE; returns
    (xs, x0_preds) as lists of host tensors, xs[0] being the input.

    Built on this package's sampler primitives: every coefficient is a host scalar looked up in one alpha-bar table
    (no per-step device cumprod, no device->host sync), every update is one fused ``a x + b y + c z`` launch, and the
    state stays on ``x``'s device (the reference hard-codes 'cuda')."""
    abar = _alpha_bar_table(b)
    eta = float(kwargs.get("eta", 0))
    n = x.size(0)
    xs, x0_preds = [x], []
    cur = x
    with torch.no_grad():
        for i, j in _legacy_grid(seq):
            at, an = abar[i + 1], abar[j + 1]
            t = torch.full((n,), float(i), device=cur.device)
            et = model({"img": img, "input": cur}, t)
            x0_t = _lincomb(cur, at ** -0.5, et, -((1.0 - at) / at) ** 0.5)
            c1 = eta * ((1.0 - at / an) * (1.0 - an) / (1.0 - at)) ** 0.5
            c2 = ((1.0 - an) - c1 * c1) ** 0.5
            cur = (_lincomb(x0_t, an ** 0.5, torch.randn_like(cur), c1, et, c2) if c1 != 0.0
                   else _lincomb(x0_t, an ** 0.5, et, c2))
            x0_preds.append(x0_t.cpu())
            xs.append(cur.cpu())
    return xs, x0_preds


def ddpm_steps(x, seq, model, b, **kwargs):
    """Legacy ancestral loop, call surface of R/util/denoising.py:35-69: ``model(x, t)`` predicts NOISE; x0 is clamped to
    [-1, 1]; returns (xs, x0_preds) as host tensors.  Same construction as ``generalized_steps``: host-scalar
    coefficients from one alpha-bar table, fused launches; the clamp is the only tensor op besides them."""
    abar = _alpha_bar_table(b)
    n = x.size(0)
    xs, x0_preds = [x], []
    cur = x
    with torch.no_grad():
        for i, j in _legacy_grid(seq):
            at, am = abar[i + 1], abar[j + 1]
            beta_t = 1.0 - at / am
            t = torch.full((n,), float(i), device=cur.device)
            e = model(cur, t)
            x0 = _lincomb(cur, (1.0 / at) ** 0.5, e, -(1.0 / at - 1.0) ** 0.5).clamp_(-1.0, 1.0)
            k0, kx = am ** 0.5 * beta_t / (1.0 - at), (1.0 - beta_t) ** 0.5 * (1.0 - am) / (1.0 - at)
            if i == 0:      # no noise on the step that lands on t = 0 (the reference multiplies by a zero mask)
                cur = _lincomb(x0, k0, cur, kx)
            else:
                cur = _lincomb(x0, k0, cur, kx, torch.randn_like(cur), beta_t ** 0.5)
            x0_preds.append(x0.cpu())
            xs.append(cur.cpu())
    return xs, x0_preds
