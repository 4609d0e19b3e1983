"""Accent discriminator of joint_train.py --multitask / --adversarial: modules/discriminator.py (`Discriminator`),
utils/functions.py:73-99,267-290,353-358 (`save_discriminator`, `load_discriminator`, `init_discriminator_model`) and
utils/metrics.py:164-199 (`calculate_adversarial`, `calculate_multi_task`) with the reference's names and signatures.

The compute is csrc/mtl_disc.hip (include/mtl_hip.h "accent discriminator"): the time sum of the encoder output, the Linear, both
losses and every gradient down to the encoder-output gradient.  Parameters and gradients are views into one flat buffer each, like
the models', so the kernels write the gradients in place.  There is no CPU path: compute on a CPU module raises.
"""
import logging
import os

import torch
import torch.nn as nn

from . import _lib

check = _lib.check
MAX_CLASSES = 64            # include/mtl_hip.h: 1 <= C <= 64


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _need_device(t, what):
    if t.device.type != 'cuda':
        raise RuntimeError('%s lives on %s: the product path needs an MI355X (call .cuda()); there is no CPU fallback' % (what, t.device))


class _DiscFn(torch.autograd.Function):
    """logits = discriminator(enc.sum(1)) for enc (B, T, d): mtl_disc_fwd; the backward writes the parameter gradients into the
    module's flat gradient buffer and returns the gradient of enc (mtl_disc_bwd_dlogits)."""

    @staticmethod
    def forward(ctx, anchor, disc, enc):
        B, T, d = enc.shape
        enc = enc.contiguous().float()
        logits = torch.empty((B, disc.num_class), dtype=torch.float32, device=enc.device)
        pooled = torch.empty((B, d), dtype=torch.float32, device=enc.device)
        disc._pool_logits(enc.data_ptr(), B, T, logits, pooled)
        ctx.disc, ctx.pooled, ctx.dims = disc, pooled, (B, T, d)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        disc, (B, T, d) = ctx.disc, ctx.dims
        disc._sync_grad_views()
        denc = torch.zeros((B, T, d), dtype=torch.float32, device=dlogits.device)
        disc.backward_from_dlogits(ctx.pooled, dlogits.contiguous().float(), B, T, denc.data_ptr())
        return None, None, denc


class Discriminator(nn.Module):
    """Discriminator for adversarial training and multi-task learning (modules/discriminator.py): one Linear(feat_dim, num_class)
    on the time sum of the encoder output.  State-dict keys `linear.weight` / `linear.bias`; the same RNG draws as nn.Linear."""

    def __init__(self, feat_dim, num_class):
        super().__init__()
        if not 1 <= int(num_class) <= MAX_CLASSES or int(feat_dim) % 4 != 0 or int(feat_dim) < 4:
            raise ValueError('Discriminator: 1 <= num_class <= %d and feat_dim %% 4 == 0 (got %d, %d)' % (MAX_CLASSES, num_class, feat_dim))
        self.feat_dim, self.num_class = int(feat_dim), int(num_class)
        self.linear = nn.Linear(feat_dim, num_class)
        self.copy_grad = None
        self._theta = self._gflat = self._anchor = None
        self._flatten()

    # ------------------------------------------------------------------ flat storage (weight | bias)
    def _flatten(self):
        w, b = self.linear.weight, self.linear.bias
        n = w.numel()
        theta = torch.zeros(n + b.numel(), dtype=torch.float32, device=w.device)
        gflat = torch.zeros_like(theta)
        for p, lo, hi in ((w, 0, n), (b, n, n + b.numel())):
            v = theta[lo:hi].view(p.shape)
            v.copy_(p.data)
            p.data = v
            g = gflat[lo:hi].view(p.shape)
            if p.grad is not None:                      # a module that moves keeps what it has accumulated
                g.copy_(p.grad)
            p.grad = g
        self._theta, self._gflat = theta, gflat
        if self.copy_grad is not None:
            self.copy_grad = [c.to(w.device) for c in self.copy_grad]
        self._anchor = torch.zeros((), device=w.device, requires_grad=True)
        self._bufs = {}

    def _apply(self, fn, *a, **kw):
        """.cuda() / .cpu() / .to(...): the flat buffers are rebuilt on the new device with the parameters', gradients' and
        copy_grad's values; an _apply that leaves the storage where it is (.float(), .share_memory(), ...) changes nothing."""
        out = super()._apply(fn, *a, **kw)
        w = self.linear.weight
        if w.device != self._theta.device or w.dtype != torch.float32 or w.data_ptr() != self._theta.data_ptr():
            self._flatten()
        return out

    @property
    def flat_parameters(self):
        return self._theta

    @property
    def flat_grad(self):
        return self._gflat

    def _sync_grad_views(self):
        """torch optimizers' zero_grad(set_to_none=True) drops the .grad views: treat that as 'gradient is zero'."""
        w = self.linear.weight
        if w.grad is None or w.grad.data_ptr() != self._gflat.data_ptr() or self.linear.bias.grad is None:
            n = w.numel()
            self._gflat.zero_()
            w.grad = self._gflat[:n].view(w.shape)
            self.linear.bias.grad = self._gflat[n:].view(self.linear.bias.shape)

    def zero_grad(self, set_to_none=False):
        self._sync_grad_views()
        self._gflat.zero_()

    # ------------------------------------------------------------------ device calls
    def _buf(self, name, shape):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = torch.empty(shape, dtype=torch.float32, device=self._theta.device)
            self._bufs[name] = t
        return t

    def _pool_logits(self, enc_ptr, B, T, logits, pooled, accent_id=0, mode=0, losses=None):
        """mtl_disc_fwd on the (B, T, d) tensor at enc_ptr -> pooled (B, d), logits (B, C), losses (2,)"""
        _need_device(self._theta, 'the discriminator')
        d, C, L = self.feat_dim, self.num_class, _lib.lib()
        nbytes = L.mtl_disc_workspace(B, T, d)
        ws = self._bufs.get('ws')
        if ws is None or ws.numel() * 4 < nbytes:
            ws = self._bufs['ws'] = torch.empty(nbytes // 4 + nbytes // 8, dtype=torch.float32, device=self._theta.device)
        if losses is None:
            losses = self._buf('losses_scratch', (2,))
        check(L.mtl_disc_fwd(_stream(self._theta.device), enc_ptr, B, T, d, self._theta.data_ptr(), self._theta.data_ptr() + 4 * C * d,
                             C, int(accent_id), int(mode), pooled.data_ptr(), logits.data_ptr(), losses.data_ptr(), ws.data_ptr(),
                             ws.numel() * 4), 'mtl_disc_fwd')

    def head_forward(self, enc, accent_id, adversarial):
        """The trainer's fused head on the engine's encoder output (B, T', d): -> losses (2,) device tensor [CE, MSE to 1/C]; pooled and
        logits stay in the module's buffers for head_backward."""
        B, T, d = enc.shape
        if d != self.feat_dim or not enc.is_contiguous():
            raise ValueError('encoder output (B, T, %d) expected, contiguous' % self.feat_dim)
        pooled, logits, losses = self._buf('pooled', (B, d)), self._buf('logits', (B, self.num_class)), self._buf('losses', (2,))
        self._pool_logits(enc.data_ptr(), B, T, logits, pooled, accent_id, 1 if adversarial else 0, losses)
        self._head = (B, T, int(accent_id), 1 if adversarial else 0)
        return losses

    def head_backward(self, a, b, denc):
        """gradient of a * CE + b * MSE of the last head_forward: += into the flat gradient and into denc (B * T', d)"""
        B, T, accent_id, mode = self._head
        self._sync_grad_views()
        C, d = self.num_class, self.feat_dim
        check(_lib.lib().mtl_disc_bwd(_stream(self._theta.device), self._bufs['pooled'].data_ptr(), self._bufs['logits'].data_ptr(),
                                      self._theta.data_ptr(), accent_id, B, T, d, C, mode, float(a), float(b), self._gflat.data_ptr(),
                                      self._gflat.data_ptr() + 4 * C * d, denc.data_ptr()), 'mtl_disc_bwd')

    def backward_from_dlogits(self, pooled, dlogits, B, T, denc_ptr):
        C, d = self.num_class, self.feat_dim
        check(_lib.lib().mtl_disc_bwd_dlogits(_stream(self._theta.device), pooled.data_ptr(), dlogits.data_ptr(), self._theta.data_ptr(),
                                              B, T, d, C, self._gflat.data_ptr(), self._gflat.data_ptr() + 4 * C * d, denc_ptr),
              'mtl_disc_bwd_dlogits')

    def forward(self, inputs):
        """inputs: B x H (the time sum of the encoder output) -> predictions: B x C.  A (B, T, H) input is summed over T first, in
        the same launches: discriminator(enc) == discriminator(torch.sum(enc, dim=1))."""
        _need_device(self._theta, 'the discriminator')
        if inputs.dim() == 2:
            inputs = inputs.unsqueeze(1)
        if inputs.dim() != 3 or inputs.shape[2] != self.feat_dim:
            raise ValueError('expected (B, %d) or (B, T, %d) inputs' % (self.feat_dim, self.feat_dim))
        return _DiscFn.apply(self._anchor, self, inputs)

    # ------------------------------------------------------------------ copy_grad API (modules/discriminator.py:26-62)
    def init_copy_grad_(self):
        self.copy_grad = [torch.zeros(p.shape, device=p.device, requires_grad=False) for p in self.parameters()]
        return self.copy_grad

    def zero_copy_grad(self):
        if self.copy_grad is None:
            self.init_copy_grad_()
        else:
            for g in self.copy_grad:
                g.zero_()

    def add_copy_grad(self):
        if self.copy_grad is None:
            self.init_copy_grad_()
        self._sync_grad_views()
        for g, p in zip(self.copy_grad, self.parameters()):
            g += p.grad

    def to_copy_grad(self):
        if self.copy_grad is None:
            self.init_copy_grad_()
        self._sync_grad_views()
        for g, p in zip(self.copy_grad, self.parameters()):
            g.copy_(p.grad)

    def from_copy_grad(self):
        if self.copy_grad is None:
            self.init_copy_grad_()
        self._sync_grad_views()
        for g, p in zip(self.copy_grad, self.parameters()):
            p.grad.copy_(g)


# ---------------------------------------------------------------------------------------------------------------------
# losses on arbitrary device logits (utils/metrics.py:164-199)
# ---------------------------------------------------------------------------------------------------------------------
class _DiscLossFn(torch.autograd.Function):
    """(CE(pred, [accent_id] * B), MSE(pred, 1/C)) by mtl_disc_loss_fwd; the backward is mtl_disc_loss_bwd once per loss that has
    an incoming gradient, scaled by it."""

    @staticmethod
    def forward(ctx, pred, accent_id, mode):
        p = pred.detach().contiguous().float()
        B, C = p.shape
        losses = torch.zeros(2, dtype=torch.float32, device=p.device)
        check(_lib.lib().mtl_disc_loss_fwd(_stream(p.device), p.data_ptr(), B, C, int(accent_id), int(mode), losses.data_ptr()),
              'mtl_disc_loss_fwd')
        ctx.save_for_backward(p)
        ctx.accent_id, ctx.mode = int(accent_id), int(mode)
        return losses[0].clone(), losses[1].clone()

    @staticmethod
    def backward(ctx, g_ce, g_mse):
        (p,) = ctx.saved_tensors
        B, C = p.shape
        L, st = _lib.lib(), _stream(p.device)
        out = torch.empty_like(p)
        check(L.mtl_disc_loss_bwd(st, p.data_ptr(), B, C, ctx.accent_id, ctx.mode, 1.0, 0.0, out.data_ptr()), 'mtl_disc_loss_bwd')
        grad = out * g_ce
        if ctx.mode == 1:
            out2 = torch.empty_like(p)
            check(L.mtl_disc_loss_bwd(st, p.data_ptr(), B, C, ctx.accent_id, ctx.mode, 0.0, 1.0, out2.data_ptr()), 'mtl_disc_loss_bwd')
            grad = grad + out2 * g_mse
        return grad, None, None


def _check_pred(pred, accent_id):
    if pred.dim() != 2:
        raise ValueError('pred: (B, C) logits expected')
    _need_device(pred, 'pred')
    if not 1 <= pred.shape[1] <= MAX_CLASSES or not 0 <= int(accent_id) < pred.shape[1]:
        raise ValueError('1 <= C <= %d classes and 0 <= accent_id < C (got C = %d, accent_id = %d)' % (MAX_CLASSES, pred.shape[1], accent_id))


def calculate_adversarial(pred, accent_id):
    """pred: prediction for one batch (B x C), accent_id: accent id of this batch -> (discriminator_loss, encoder_loss)
    = (F.cross_entropy(pred, [accent_id] * B), F.mse_loss(pred, 1/C))      (utils/metrics.py:164-183)"""
    _check_pred(pred, accent_id)
    return _DiscLossFn.apply(pred, int(accent_id), 1)


def calculate_multi_task(pred, accent_id):
    """-> discriminator_loss = F.cross_entropy(pred, [accent_id] * B)      (utils/metrics.py:185-199)"""
    _check_pred(pred, accent_id)
    return _DiscLossFn.apply(pred, int(accent_id), 0)[0]


# ---------------------------------------------------------------------------------------------------------------------
# factory and checkpoints (utils/functions.py)
# ---------------------------------------------------------------------------------------------------------------------
def init_discriminator_model(args):
    return Discriminator(args.dim_model, args.num_class)


def save_discriminator(discriminator, epoch, opt, args, best_model=False):
    """utils/functions.py:73-99: the dict {'args', 'epoch', 'model_state_dict', 'opt'} with the torch.optim object pickled whole.
    best_discriminator.th keeps the reference's name; the periodic checkpoint goes to epoch_N_discriminator.th (the reference writes
    it to epoch_N.th, over the model checkpoint it has just saved there).  Tensors are stored on the CPU so both stacks can read it."""
    folder = '{}/{}'.format(args.save_folder, args.name)
    save_path = folder + ('/best_discriminator.th' if best_model else '/epoch_{}_discriminator.th'.format(epoch))
    os.makedirs(folder, exist_ok=True)
    print('SAVE DISCRIMINATOR to', save_path)
    logging.info('SAVE DISCRIMINATOR to ' + save_path)
    state = {k: v.detach().cpu().clone() for k, v in discriminator.state_dict().items()}
    params = [torch.nn.Parameter(state[n], requires_grad=True) for n, _ in discriminator.named_parameters()]
    sd = opt.state_dict()           # (its per-parameter dicts are the optimizer's own: copy, never edit in place)
    sd = {'param_groups': sd['param_groups'],
          'state': {i: {k: v.detach().cpu().clone() if torch.is_tensor(v) else v for k, v in st.items()} for i, st in sd['state'].items()}}
    out_opt = type(opt)(params, lr=opt.param_groups[0]['lr'])
    out_opt.load_state_dict(sd)
    torch.save({'args': args, 'epoch': epoch, 'model_state_dict': state, 'opt': out_opt}, save_path)
    return save_path


def load_discriminator(load_path, train=True):
    """utils/functions.py:267-290 -> (discriminator, opt): the optimizer comes back as torch.optim.Adam holding the saved state
    (built at args.lr like the reference does, then overwritten by the saved parameter groups)."""
    ckpt = torch.load(load_path, map_location=torch.device('cpu'), weights_only=False)
    args = ckpt['args']
    discriminator = init_discriminator_model(args)
    discriminator.load_state_dict(ckpt['model_state_dict'])
    discriminator = discriminator.cuda() if getattr(args, 'cuda', False) and torch.cuda.is_available() else discriminator.cpu()
    opt = torch.optim.Adam(discriminator.parameters(), lr=args.lr)
    opt.load_state_dict(ckpt['opt'].state_dict())
    return discriminator, opt
