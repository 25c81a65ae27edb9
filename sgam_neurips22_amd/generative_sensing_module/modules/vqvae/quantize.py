"""VectorQuantizer2 on the HIP backend — same constructor / attributes / return structure as the reference
(sgam/generative_sensing_module/modules/vqvae/quantize.py:213-381).

forward                : L2 nearest codeword (MFMA z.e^T + exact-order distance/arg-min kernel), embedding
                         gather, straight-through value z + (z_q - z)            (reference :275-319)
get_multiple_codewords : top-k infill sampler (reference :344-381) — distances / top-k on the GPU, the
                         softmax + multinomial draws on the host CPU generator: draw for draw what the reference's
                         CPU path does (the parity target of this backend; pinned by tests/golden/vqgan_topk4_s2.npz),
                         including its quirk of sampling every token from row 0's distribution (:358).  A reference
                         run with the model on a CUDA device draws from the device generator instead, so against
                         such a run the parity is statistical only.
DeviceInfillSampler    : the second sampler, next to the host one: the same draws rule evaluated on the GPU with a counter-based
                         generator (ops.vq_sample_topk; DESIGN "Device-side top-k infill sampler") — no host round trip, so a
                         sampling forward replays as a captured graph.  Installed by VQModel.set_infill_sampler("device").
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .... import ops


class DeviceInfillSampler:
    """State of the device-side top-k infill sampler: the configuration (seed, per-token mode, temperature) and, per batch
    size, ONE persistent device buffer [call lo32, call hi32, stream id 0 .. B-1] (int32) that the kernel reads by address.
    `begin` writes the values of the coming forward into a pinned staging slot and copies the slot to the buffer
    asynchronously on the current stream (a ring of slots, so that the host never rewrites a slot whose copy has not run);
    every launch between `begin` and `end` — warm-up, capture, replay, the range guard's recompute — draws with that call
    number.  `end` advances the call number by one."""

    RING = 8

    def __init__(self, seed=0, per_token=False, temperature=1.0):
        if not temperature > 0:
            raise ValueError(f"infill sampler temperature must be positive, not {temperature!r}")
        self.seed, self.per_token, self.temperature = int(seed), bool(per_token), float(temperature)
        self.call = 0
        self.streams = None          # None: batch item b draws from stream b
        self.armed = False
        self._bufs = {}              # (B, device) -> [device buffer, pinned slots, their copy-done events, next slot]

    def begin(self, B, device):
        ids = list(range(B)) if self.streams is None else [int(v) for v in self.streams]
        if len(ids) != B:
            raise ValueError(f"infill sampler: {len(ids)} stream ids for a batch of {B}")
        ent = self._bufs.get((B, str(device)))
        if ent is None:
            ent = self._bufs[(B, str(device))] = [
                torch.zeros(2 + B, dtype=torch.int32, device=device),
                [torch.zeros(2 + B, dtype=torch.int32).pin_memory() for _ in range(self.RING)], [None] * self.RING, 0]
        buf, slots, done, i = ent
        ent[3] = (i + 1) % self.RING
        if done[i] is not None:
            done[i].synchronize()    # only ever waits when the host is a whole ring ahead
        call = int(self.call) & 0xFFFFFFFFFFFFFFFF
        words = np.array([call & 0xFFFFFFFF, call >> 32] + [v & 0xFFFFFFFF for v in ids], dtype=np.uint32)
        slots[i].copy_(torch.from_numpy(words.view(np.int32)))
        buf.copy_(slots[i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        done[i] = ev
        self.armed = True
        self._cur = buf

    def end(self):
        self.armed = False
        self.call = int(self.call) + 1

    def buffers(self):
        """(call, stream_id) views of the armed forward's device buffer"""
        return self._cur[:2], self._cur[2:]


class VectorQuantizer2(nn.Module):
    def __init__(self, n_e, e_dim, beta, remap=None, unknown_index="random", sane_index_shape=False, legacy=True,
                 kmean_init_codebook_path=None):
        super().__init__()
        self.n_e, self.e_dim, self.beta, self.legacy = n_e, e_dim, beta, legacy
        self.kmean_init_codebook_path = kmean_init_codebook_path
        self.embedding = nn.Embedding(n_e, e_dim)
        if kmean_init_codebook_path is None:
            self.embedding.weight.data.uniform_(-1.0 / n_e, 1.0 / n_e)
        else:
            self.embedding.weight.data.copy_(torch.from_numpy(np.load(kmean_init_codebook_path)))
        if remap is not None:
            raise NotImplementedError("index remapping is unused by SGAM (remap=None in every config)")
        self.remap = None
        self.re_embed = n_e
        self.sane_index_shape = sane_index_shape
        self.consume_host_rng = False
        self.device_sampler = None          # a DeviceInfillSampler, or None: the host sampler (the reference's CPU draws)

    # ---- codebook cache: contiguous fp32 copy + |e|^2, refreshed when the weight changes ----
    def _codebook(self):
        w = self.embedding.weight
        key = (w.data_ptr(), w._version, str(w.device))
        if getattr(self, "_cb_key", None) != key:
            self._cb = w.detach().float().contiguous()
            self._cb_sq = ops.row_sumsq(self._cb)
            self._cb_key = key
        return self._cb, self._cb_sq

    def quantize_nhwc(self, z_nhwc, want_dist=False):
        """z (B,h,w,D) -> (z_q (B,h,w,D) straight-through value, idx (B,h,w) int64, dist or None)."""
        B, h, w, D = z_nhwc.shape
        cb, cb_sq = self._codebook()
        idx, zq, dist = ops.vq_nearest(z_nhwc.reshape(B * h * w, D), cb, cb_sq, straight_through=True,
                                       want_dist=want_dist)
        return zq.view(B, h, w, D), idx.view(B, h, w), dist

    def commit_loss_nhwc(self, z_nhwc, idx):
        """the `loss` of reference forward (:296-301, legacy): mean((z_q-z)^2) + beta*mean((z_q-z)^2), 0-d fp32 tensor"""
        D = z_nhwc.shape[-1]
        return ops.vq_commit_loss(z_nhwc.reshape(-1, D), self._codebook()[0], idx, self.beta)

    def forward(self, z, temp=None, rescale_logits=False, return_logits=False, encoding_indices=None, valid_mask=None):
        assert temp is None or temp == 1.0, "Only for interface compatible with Gumbel"
        assert rescale_logits is False, "Only for interface compatible with Gumbel"
        assert return_logits is False, "Only for interface compatible with Gumbel"
        zn = ops.nchw_to_nhwc(z)
        if encoding_indices is None:
            zq, idx, _ = self.quantize_nhwc(zn)
        else:
            B, h, w, D = zn.shape
            idx = encoding_indices.reshape(B, h, w)
            zq = ops.vq_gather(self._codebook()[0], idx).view(B, h, w, D)
        loss = self.commit_loss_nhwc(zn, idx)
        if self.sane_index_shape:
            idx = idx.reshape(zq.shape[0], zq.shape[1], zq.shape[2])
        return ops.nhwc_to_nchw(zq), loss, (None, None, idx)

    def get_codebook_entry(self, indices, shape):
        zq = ops.vq_gather(self._codebook()[0], indices.reshape(-1))
        if shape is not None:
            zq = ops.nhwc_to_nchw(zq.view(shape))
        return zq

    def update_codebook(self, features, codebook_indices):
        w = self.embedding.weight.data
        for i, ci in enumerate(codebook_indices):
            w[ci] = torch.from_numpy(features[i]).to(w.device)
        self.embedding.weight.data.copy_(w)

    def sample_nhwc(self, z_nhwc, topk, sample_number, extrapolation_mask):
        """get_multiple_codewords on an NHWC latent.  Returns z_qs (B,S,h,w,D) NHWC-per-sample and indices (B,S,h,w).

        For B = 1 and a 16x16 latent this is the reference (:344-381) draw for draw, including its quirk that every
        token samples from the distribution of token 0.  The reference hard-codes B = 1 / 16x16 (:345, :368, :381);
        larger batches and latents are this backend's generalisation (candidate batching): batch items
        are processed in order, each exactly like a B = 1 call (its own token-0 distribution, its own h*w consecutive
        CPU-RNG draws, its mask resized to (h, w)), so a batch equals the same items run one after the other."""
        B, h, w, D = z_nhwc.shape
        dev = z_nhwc.device
        cb, cb_sq = self._codebook()
        T = h * w
        if topk == 1 and not self.consume_host_rng:
            # softmax over one candidate is 1.0 and multinomial can only return slot 0: every token gets its
            # arg-min whatever the mask says, so nothing has to leave the GPU (the reference's 256 CPU draws
            # per frame change no output; set consume_host_rng=True to also advance the CPU RNG like it does).
            if sample_number == 1:
                # one sample per token: the arg-min launch writes the chosen codebook row itself (no straight-through
                # arithmetic: get_multiple_codewords returns the embedding, :381) — no gather launch
                idx1, zq, _ = ops.vq_nearest(z_nhwc.reshape(B * T, D), cb, cb_sq, straight_through=False, want_zq=True)
                return zq.view(B, 1, h, w, D), idx1.view(B, 1, h, w)
            idx1, _, _ = ops.vq_nearest(z_nhwc.reshape(B * T, D), cb, cb_sq, want_zq=False)
            sampled = idx1.view(B, T, 1).expand(-1, -1, sample_number)
        elif self.device_sampler is not None:
            # second sampler: candidates, weights, Philox draw, mask and gather on the GPU (ops.vq_sample_topk) — nothing
            # crosses to the host, so this forward can be captured and replayed
            ds = self.device_sampler
            own = not ds.armed          # called outside VQModel.forward (encode / get_multiple_codewords): its own call
            if own:
                ds.begin(B, dev)
            try:
                call, stream_id = ds.buffers()
                _, _, dist = ops.vq_nearest(z_nhwc.reshape(B * T, D), cb, cb_sq, want_dist=True, want_zq=False)
                zq, idx, _, _ = ops.vq_sample_topk(dist, cb, topk, sample_number, (h, w), stream_id, call, seed=ds.seed,
                                                   mask=extrapolation_mask, per_token=ds.per_token,
                                                   temperature=ds.temperature)
            finally:
                if own:
                    ds.end()
            return zq, idx
        else:
            idx1, _, dist = ops.vq_nearest(z_nhwc.reshape(B * T, D), cb, cb_sq, want_dist=True, want_zq=False)
            vals, tk_idx = ops.vq_topk(dist, topk)
            vals_h = vals.view(B, T, topk)[:, 0].cpu()                           # token 0 of every item
            em_all = extrapolation_mask.reshape(B, 1, *extrapolation_mask.shape[-2:]).float().cpu()
            draws = []
            for b in range(B):
                # host side, CPU RNG stream — identical draws to the reference (row 0's distribution for all tokens)
                dist0 = F.softmax(-vals_h[b] / 1, dim=-1)
                d = torch.stack([torch.multinomial(dist0, sample_number, replacement=True) for _ in range(T)])
                em = F.interpolate(em_all[b:b + 1], size=(h, w)).view(-1)
                d[(1 - em) != 0] = 0  # outside the hole: arg-min (= top-1)
                draws.append(d)
            draws = torch.stack(draws).to(dev)                                   # (B, T, S)
            sampled = torch.gather(tk_idx.view(B, T, topk), 2, draws)            # (B, T, S)
        order = sampled.permute(0, 2, 1).contiguous()                            # (B, S, T)
        zq = ops.vq_gather(cb, order.reshape(-1))                                # (B*S*T, D), pure gather
        return zq.view(B, sample_number, h, w, D), order.reshape(B, sample_number, h, w)

    def get_multiple_codewords(self, z, topk=10, sample_number=1, extrapolation_mask=None, return_exp_probility=None,
                               temp=1):
        zqs, idx = self.sample_nhwc(ops.nchw_to_nhwc(z), topk, sample_number, extrapolation_mask)
        S = zqs.shape[1]
        out = torch.stack([ops.nhwc_to_nchw(zqs[:, i].contiguous()) for i in range(S)], 1)  # (B,S,D,h,w)
        return out, None, (None, None, idx)
