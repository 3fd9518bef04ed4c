"""Drop-in `GaussianDiffusion` (pose_diffusion/models/gaussian_diffuser.py:75-341).

Same constructor, same 13 persistent buffers (checkpoint keys `diffuser.betas` ...), same
``sample(shape, z, cond_fn=None, cond_start_step=0) -> (pose [B,N,9], process [T+1,B,N,9])``.
The loop itself -- 100 denoiser evaluations, posterior updates and (when cond_fn is the shipped
GGS partial) the 7000 guided iterations -- runs as one hipGraph replay of hand-written kernels.
The training branch (`forward` / `p_losses`, :308-332) runs on the engine, one pass of the denoiser for the whole batch of per-sequence
timesteps.  By default (``engine_grad = False``) it is the FORWARD half only: the diffusion loss of a checkpoint on a batch, no grad.
With ``engine_grad = True`` and grad mode on, the loss comes from the trainer (posediffusion_amd/train.py, include/pd_engine_train.h)
and is attached to the denoiser's parameters (and to z when it requires grad): ``loss.mean().backward()`` runs the hand-written
backward, PyTorch keeps the optimiser.  By default the network is evaluated as under ``model.eval()``: the reference under
``model.train()`` applies dropout, so with ``engine_dropout = False`` engine training is dropout-0 training and the opt-in refuses a
diffuser in ``.train()`` mode whose encoder layers have dropout p > 0.  ``engine_dropout = True`` (a second opt-in, under
``engine_grad``) trains the model as built: in ``.train()`` mode the trainer applies the encoder layers' dropout p at their four sites
with masks of its own counter-based generator -- one int64 seed per call from torch's default CPU generator, so ``torch.manual_seed``
reproduces a run -- and differentiates that function.  The masks are not torch's: the distribution is the reference's, the bits are not.
``engine_grad_outputs = True`` (a third opt-in, under ``engine_grad``) returns ``x_0_pred`` with its graph, as the reference's ``p_losses``
does: any loss written on it -- or on the ``pred_cameras`` that ``PoseDiffusionModel.forward(..., training=True)`` decodes from it -- flows
back into the denoiser and z (pd_train_backward_ex, pd_pose_to_camera_backward).  The trainer keeps ONE stash: every such term must be
part of the one total whose ``.backward()`` follows the call.  ``x_t`` stays data.
The trainer takes sequences of up to 64 frames by default; ``engine_grad_max_frames`` (64 .. 256) raises that (PD_TR_OPT_MAX_FRAMES:
above 64 frames the attention and its backward run key-tiled kernels).
``n_frames=`` on ``p_losses`` / ``forward`` (this package's extension): [B] frame counts of a padded batch -- sequence b has n_frames[b]
frames in rows 0 .. of its N-row block, padding rows of ``x_start``, ``z`` and ``noise`` are never read and padding rows of the results
are +0.  Such a call goes through the trainer in either grad mode (the engine's forward-only path takes uniform batches): with
``engine_grad`` and grad mode on the loss is differentiable, otherwise it is the trainer's forward alone.  ``loss`` is [B, N, 9] with +0
at padding, so the reference's ``loss.mean()`` divides by the padded size; the mean over real frames is
``loss.sum() / (9 * sum(n_frames))``."""
import os
from collections import namedtuple

import torch
from torch import nn

from posediffusion_amd import host
from posediffusion_amd.schedule import BUFFER_NAMES, diffusion_buffers


ModelPrediction = namedtuple("ModelPrediction", ["pred_noise", "pred_x_start"])      # gaussian_diffuser.py:34


def _at(table, t, like):
    """table[t] broadcast over the trailing axes of ``like`` (the reference's ``extract``, :49-52); t: int or LongTensor [B]."""
    t = torch.as_tensor(t, device=table.device, dtype=torch.long).reshape(-1)
    return table[t].reshape((-1,) + (1,) * (like.dim() - 1))


class GaussianDiffusion(nn.Module):
    def __init__(self, timesteps=100, sampling_timesteps=None, beta_1=0.0001, beta_T=0.1, loss_type="l1",
                 objective="pred_noise", beta_schedule="custom", p2_loss_weight_gamma=0.0, p2_loss_weight_k=1):
        super().__init__()
        if objective not in {"pred_noise", "pred_x0"}:
            raise AssertionError("objective must be either pred_noise (predict noise) or pred_x0 (predict image start)")
        self.objective, self.loss_type, self.beta_schedule = objective, loss_type, beta_schedule
        self.timesteps, self.beta_1, self.beta_T = timesteps, beta_1, beta_T
        bufs = diffusion_buffers(beta_schedule, timesteps, beta_1, beta_T, p2_loss_weight_gamma, p2_loss_weight_k)
        for name in BUFFER_NAMES:
            self.register_buffer(name, bufs[name])
        self.num_timesteps = int(timesteps)
        self.sampling_timesteps = timesteps if sampling_timesteps is None else sampling_timesteps
        assert self.sampling_timesteps <= timesteps
        self.model = None          # the Denoiser, assigned after construction (pose_diffusion_model.py:61)
        self.use_graph = os.environ.get("PD_USE_GRAPH", "1") != "0"
        self.last_ggs_stats = None
        self.ggs_max_frames = host.GGS_MAX_FRAMES      # frames guided sampling admits; raise it (<= 256) to guide longer sequences: the engine
        #                                                then holds a larger exchange region (PD_OPT_GGS_MAX_FRAMES, include/pd_engine.h)
        self.engine_grad = False                       # True: with grad mode on, p_losses / forward return a loss that is differentiable with respect to the
        #                                                denoiser's parameters and z (the trainer's hand-written backward); the default stays forward-only
        self.engine_grad_max_frames = 64               # frames per sequence engine_grad admits; raise it (<= 256) to train on longer sequences (PD_TR_OPT_MAX_FRAMES)
        self.engine_dropout = False                    # True (with engine_grad, in .train() mode): the trainer applies the encoder layers' dropout instead of refusing it
        self.engine_grad_outputs = False               # True (with engine_grad): x_0_pred is differentiable too, so a loss on it or on the cameras decoded from it flows back
        self.ggs_long_pair_items = False               # True: above 64 frames, take frame pairs of more than 512 matches (PD_OPT_GGS_LONG_PAIR_ITEMS)

    # ---- schedule helpers (:190-216): elementwise on the buffers, same names and argument order; the sampler itself has these
    # fused into pd_tail_kernel and does not call them
    def predict_start_from_noise(self, x_t, t, noise):
        return _at(self.sqrt_recip_alphas_cumprod, t, x_t) * x_t - _at(self.sqrt_recipm1_alphas_cumprod, t, x_t) * noise

    def predict_noise_from_start(self, x_t, t, x0):
        return (_at(self.sqrt_recip_alphas_cumprod, t, x_t) * x_t - x0) / _at(self.sqrt_recipm1_alphas_cumprod, t, x_t)

    def q_posterior(self, x_start, x_t, t):
        mean = _at(self.posterior_mean_coef1, t, x_t) * x_start + _at(self.posterior_mean_coef2, t, x_t) * x_t
        return mean, _at(self.posterior_variance, t, x_t), _at(self.posterior_log_variance_clipped, t, x_t)

    def q_sample(self, x_start, t, noise=None):
        noise = torch.randn_like(x_start) if noise is None else noise
        return _at(self.sqrt_alphas_cumprod, t, x_start) * x_start + _at(self.sqrt_one_minus_alphas_cumprod, t, x_start) * noise

    def model_predictions(self, x, t, z, x_self_cond=None):
        """(:218-229) one denoiser evaluation on the engine; the pair (pred_noise, pred_x_start) by the objective."""
        out = self.model(x, t, z)
        if self.objective == "pred_noise":
            return ModelPrediction(out, self.predict_start_from_noise(x, t, out))
        return ModelPrediction(self.predict_noise_from_start(x, t, out), out)

    @property
    def loss_fn(self):                                              # :334-341
        if self.loss_type == "l1":
            return nn.functional.l1_loss
        if self.loss_type == "l2":
            return nn.functional.mse_loss
        raise ValueError(f"invalid loss type {self.loss_type}")

    # ---- step-level pieces (same names as the reference) ------------------------------------
    def p_mean_variance(self, x, t, z, x_self_cond=None, clip_denoised=False):
        if clip_denoised:
            raise NotImplementedError("We don't clip the output because pose does not have a clear bound.")
        B, N, _ = x.shape
        eng = host.get_engine(self.model, self, B, N)
        tt = int(torch.as_tensor(t).reshape(-1)[0])
        mean, x0 = eng.p_mean(x, z, tt)
        shape = (B,) + (1,) * (x.dim() - 1)
        return (mean, self.posterior_variance[tt].expand(shape), self.posterior_log_variance_clipped[tt].expand(shape), x0)

    @torch.no_grad()
    def p_sample(self, x, t: int, z, x_self_cond=None, clip_denoised=False, cond_fn=None, cond_start_step=0):
        B, N, _ = x.shape
        eng = host.get_engine(self.model, self, B, N)
        mean, x0 = eng.p_mean(x, z, int(t))
        if cond_fn is not None and t < cond_start_step:           # gaussian_diffuser.py:270-276
            mean = cond_fn(mean, t)
            noise = None
        else:
            noise = torch.randn_like(x) if t > 0 else None        # :278
        return eng.p_finish(mean, noise, int(t)), x0

    @torch.no_grad()
    def p_sample_loop(self, shape, z, cond_fn=None, cond_start_step=0, n_frames=None):
        """``n_frames`` (this package's extension; the reference's signature when omitted): [B] frame counts of a padded batch --
        sequence b has n_frames[b] frames in rows 0 .. of its N-row block, padding rows of the results are 0; with guidance the
        ``matches_dict`` of sequence b must come from n_frames[b] frames (``img_shape[0]``)."""
        B, N, _ = shape
        if n_frames is not None:
            n_frames = [int(v) for v in (n_frames.tolist() if hasattr(n_frames, 'tolist') else n_frames)]
            if len(n_frames) != B or min(n_frames) < 1 or max(n_frames) > N:
                raise ValueError(f"n_frames must hold one count in [1, {N}] per sequence ({B}), got {n_frames}")
        device = self.betas.device
        parsed = host.parse_ggs_cond_fn(cond_fn) if cond_fn is not None else None
        # demo.py:79-92: hloc returning no matches (kp1 is None) means sampling without GGS
        has_ggs = False
        if parsed is not None and cond_start_step > 0:
            mds = parsed[0] if isinstance(parsed[0], (list, tuple)) else [parsed[0]]
            have = [host.has_matches(m) for m in mds]
            if any(have) and not all(have):
                # guidance (and with it the noise schedule, gaussian_diffuser.py:270-278) is a property of the whole call: silently
                # dropping it for every sequence because one has no matches would change the results of the others
                raise ValueError(f"sequences {[b for b, h in enumerate(have) if not h]} of the batch have no matches: sample them in a call "
                                 "without cond_fn (demo.py:79-92) and the others with it")
            has_ggs = all(have)
        ggs_max = int(getattr(self, "ggs_max_frames", host.GGS_MAX_FRAMES))
        if has_ggs and N > ggs_max:
            # the denoiser takes up to 256 frames, GGS 64 unless ggs_max_frames was raised (include/pd_engine.h): no silent fallback to unguided sampling
            raise RuntimeError(f"guided sampling (GGS) is limited to {ggs_max} frames, got {N}: run unguided (GGS.enable=False)")
        eng = host.get_engine(self.model, self, B, N, ggs_max_frames=ggs_max if has_ggs else host.GGS_MAX_FRAMES,
                              ggs_long_pair_items=has_ggs and bool(getattr(self, "ggs_long_pair_items", False)))
        if cond_fn is not None and parsed is None and n_frames is not None:
            raise NotImplementedError("n_frames with a guidance callable other than the shipped geometry_guided_sampling partial: "
                                      "a callable sees one padded [B, N, 9] tensor and cannot know the counts")
        if cond_fn is not None and parsed is None:
            # unknown guidance callable: reference control flow in Python, arithmetic on the HIP kernels
            pose = torch.randn(shape, device=device)
            process = [pose.unsqueeze(0)]
            for t in reversed(range(self.num_timesteps)):
                pose, _ = self.p_sample(pose, t, z, cond_fn=cond_fn, cond_start_step=cond_start_step)
                process.append(pose.unsqueeze(0))
            return pose, torch.cat(process)
        noise = host.draw_noise(tuple(shape), self.num_timesteps, device, cond_start_step, has_ggs)
        cfg = None
        if has_ggs:
            matches, cfg = parsed
            host.upload_matches(eng, matches, B, n_frames)
        pose, process, stats = eng.sample(z, noise, cond_start_step if has_ggs else 0, cfg, use_graph=self.use_graph, n_frames=n_frames)
        self.last_ggs_stats = stats
        if has_ggs:
            # the GGS workgroups of a sequence exchange sums through bounded spins; one that gave up (co-residency lost
            # to another process) raises here instead of returning garbage poses, and the flag is cleared for the next call
            eng.check_async()
        # (the reference prints these lines unconditionally, geometry_guided_sampling.py:124; PD_GGS_VERBOSE=0 mutes them)
        if stats is not None and os.environ.get("PD_GGS_VERBOSE", "1") not in ("", "0"):
            st = stats.cpu()
            for k in range(st.shape[0]):
                host.print_ggs_stats(st[k], cond_start_step - 1 - k, int(dict(cfg).get("iter_num", 100)))   # incl. the drop line, :104-108
        return pose, process

    @torch.no_grad()
    def sample(self, shape, z, cond_fn=None, cond_start_step=0, n_frames=None):
        return self.p_sample_loop(shape, z=z, cond_fn=cond_fn, cond_start_step=cond_start_step, n_frames=n_frames)

    # ---- training branch, forward half (:308-332): q_sample, the denoiser and the loss as one pass on the engine ----------------------
    def _check_no_dropout(self):
        """Engine training is dropout-0 training: where the reference would apply dropout and the engine does not, refuse."""
        if not self.training:
            return
        ps = [m.p for m in self.model._trunk.modules() if isinstance(m, nn.Dropout)]
        ps += [float(getattr(l.self_attn, "dropout", 0.0)) for l in self.model._trunk.layers]
        if any(p > 0 for p in ps):
            raise RuntimeError(f"engine_grad: the diffuser is in .train() mode and its encoder layers have dropout p = {max(ps)}: the reference "
                               "would apply dropout there and the engine does not (no-dropout rule). Set TRANSFORMER.dropout = 0 or call .eval()")

    def _dropout_p(self):
        """The one dropout probability of the trunk's encoder layers (all four sites of every layer), for ``engine_dropout``."""
        ps = [float(m.p) for m in self.model._trunk.modules() if isinstance(m, nn.Dropout)]
        ps += [float(getattr(l.self_attn, "dropout", 0.0)) for l in self.model._trunk.layers]
        if not ps:
            return 0.0
        if min(ps) != max(ps):
            raise RuntimeError(f"engine_dropout: the encoder layers' dropout sites have different probabilities ({min(ps)} and {max(ps)}): "
                               "the trainer applies ONE p at the four sites of every layer")
        return ps[0]

    def _p_losses_grad(self, x_start, t, z, noise, n_frames=None, grad=True):
        """p_losses through the trainer: ``loss`` carries grad with respect to the denoiser's parameters and z.  ``grad = False`` (a call
        with ``n_frames`` under no_grad or without ``engine_grad``): the trainer's forward alone, its stash dropped."""
        from posediffusion_amd.train import check_frame_counts, p_losses_with_grad
        if n_frames is not None:
            n_frames = check_frame_counts(n_frames, x_start.shape[0], x_start.shape[1])
        if self.loss_type not in ("l1", "l2"):
            raise ValueError(f"invalid loss type {self.loss_type}")
        limit = int(getattr(self, "engine_grad_max_frames", 64))
        drop = {}
        if not getattr(self, "engine_grad", False):
            pass                                                                    # forward-only default: the eval-mode network, as on the engine
        elif self.training and getattr(self, "engine_dropout", False):
            p = self._dropout_p()
            if p > 0:                                                               # one draw per call, on the CPU: no device sync
                drop = {"dropout_p": p, "seed": int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64)), "step": 0}
        else:
            self._check_no_dropout()
        noise = torch.randn_like(x_start) if noise is None else noise              # :309
        B, N, _ = x_start.shape
        if N > limit:
            raise RuntimeError(f"engine_grad: N={N} exceeds the trainer's limit of {limit} frames per sequence; set engine_grad_max_frames = {N} "
                               "(at most 256) to train on sequences of this length")
        tr = host.get_trainer(self.model, self, B, N, max_frames=limit)
        if grad:
            if getattr(self, "engine_grad_outputs", False):
                drop["differentiable_outputs"] = True
            out = p_losses_with_grad(tr, self.model, x_start, z, t, noise, self.loss_type, n_frames=n_frames, **drop)
        else:
            with torch.no_grad():
                out = tr.forward(dict(self.model.named_parameters()), x_start, z, t, noise, self.loss_type, n_frames=n_frames, **drop)
            tr.drop_stash()
        return {"loss": out["loss"], "noise": noise, "x_0_pred": out["x_0_pred"], "x_t": out["x_t"], "t": t}

    def p_losses(self, x_start, t, z=None, noise=None, n_frames=None):
        """``{"loss", "noise", "x_0_pred", "x_t", "t"}`` as the reference returns them; loss elementwise (reduction "none").
        Eval-mode forward; no grad unless ``engine_grad`` is set and grad mode is on (see the module docstring).
        ``n_frames`` [B]: frame counts of a padded batch (module docstring); the call then runs on the trainer in either grad mode."""
        limit = int(getattr(self, "engine_grad_max_frames", 64))
        if not 64 <= limit <= 256:
            raise ValueError(f"engine_grad_max_frames = {limit} is outside [64, 256]")
        grad = getattr(self, "engine_grad", False) and torch.is_grad_enabled()
        if n_frames is not None:
            if z is None:
                raise NotImplementedError("the denoiser cannot run unconditionally: p_losses needs the image features z")
            return self._p_losses_grad(x_start, t, z, noise, n_frames=n_frames, grad=grad)
        if z is not None and grad:
            return self._p_losses_grad(x_start, t, z, noise)
        return self._p_losses_forward_only(x_start, t, z=z, noise=noise)

    @torch.no_grad()
    def _p_losses_forward_only(self, x_start, t, z=None, noise=None):
        if z is None:
            raise NotImplementedError("the denoiser cannot run unconditionally: p_losses needs the image features z")
        if self.loss_type not in ("l1", "l2"):
            raise ValueError(f"invalid loss type {self.loss_type}")
        noise = torch.randn_like(x_start) if noise is None else noise              # :309
        B, N, _ = x_start.shape
        eng = host.get_engine(self.model, self, B, N)
        out = eng.p_losses(x_start, z, t, noise, self.loss_type)
        return {"loss": out["loss"], "noise": noise, "x_0_pred": out["x_0_pred"], "x_t": out["x_t"], "t": t}

    def forward(self, pose, z=None, *args, **kwargs):
        if z is None:
            raise NotImplementedError("the denoiser cannot run unconditionally: forward needs the image features z")
        t = torch.randint(0, self.num_timesteps, (len(pose),), device=pose.device).long()      # :330-331
        return self.p_losses(pose, t, z=z, *args, **kwargs)
