"""The VGG front-end of a pass and the encoder's input Linear: everything between the input batch and e0, and between de0 and
conv0's weight gradient, as calls into libmtl_hip.so.  conv0 (1 -> 64), the three 3 x 3 layers of LAYERS, the input Linear (5120 ->
512) on the permuted weight -- or, for a model built with feat_extractor='large_cnn', the same shape at half the width: conv0 (1 -> 32),
LAYERS_LARGE, 2560 inputs (STACKS; layers_for() tells the two apart by conv0's channel count).  One table row per 3 x 3 layer, one
adapter per precision mode (which call, which argument order), one walker per direction:
  * 'f32' issues single-task calls, task by task -- layer by layer when the tasks bring frame counts of their own (`widths`), a
    layer's tails being cleared for all tasks before the next layer reads them;
  * 'x3' and 'h2' issue ONE `_tb` launch per layer for the samples of all tasks when the pass carries several tasks or `widths` (a
    single widened task takes the several-task launches too: they skip its tail rows), else the single-task call for the one task.
A model without convolutions (feat_extractor='none') takes FrameFront instead, the same five methods around csrc/mtl_featproj.hip
(front_for chooses; time_shift tells the two kinds' encoder extents apart).
PassEngine._forward_device / .backward call in here through a Front, which uses the engine's buf / scratch / colsum / gemm / _census.
A Front takes eng.lib when it is made, once per direction, as the pass itself does: bench.py and the command-list recorder swap that
attribute around whole passes.  One kept across such a swap would go on calling the library it was made with, past the recorder."""
import collections

import torch

from . import _lib
from ._lib import check
from .batchmeta import CONV_TIME_SHIFT

# the bounds max|tensor| of the h2 operands (csrc/mtl_h2.h): AMAX_PER_TASK slots of _lib.AMAX_SLOTS floats per task, raised by the
# producers' epilogues (forward), written by the bias-gradient column sums or delivered by the data-gradient epilogues (backward)
SLOT = dict(y1=0, p1=1, y5=2, dp2=3, dy5=4, dp1=5, p2=6, wp=7, de0=8)
AMAX_PER_TASK = 12
AMAX_STRIDE = AMAX_PER_TASK * _lib.AMAX_SLOTS      # floats between two tasks' bounds
CENSUS_SLOTS = 9    # slots the h2 guard counts (TransientTrainer.h2_check_every): all of SLOT but the weight's
CENSUS_NAMES = {0: 'conv0 out', 1: 'pool1', 2: 'conv5 out', 3: 'd pool2', 4: 'd conv5 out', 5: 'd pool1', 6: 'pool2', 8: 'd input-linear out'}

# one 3 x 3 layer: parameters conv.<idx>.*, cin -> cout channels, max-pooled or not, resolution level of its input (frames >> lvl: the
# `wshift` of mtl_zero_tails and of the _tb calls), arena names of input / output / arg-max bytes / gradient of the output / of the
# input, and the bound slots of those four tensors (adx None: nothing reads a bound of dy1).  own_bias: the bias gradient is always a
# column-sum pass of its own (dp2's bound has no other producer); the other layers' rides on the weight gradient where that can carry it
Layer = collections.namedtuple('Layer', 'i idx cin cout pool lvl x y am dy dx ax ay ady adx own_bias weight bias wf wd')


def _layer(i, idx, cin, cout, pool, lvl, x, y, am, dy, dx, own_bias=False):
    return Layer(i, idx, cin, cout, pool, lvl, x, y, am, dy, dx, SLOT[x], SLOT[y], SLOT[dy[1:]], SLOT.get(dx[1:]), own_bias, 'conv.%d.weight' % idx,
                 'conv.%d.bias' % idx, 'wf%d' % idx, 'wd%d' % idx)


LAYERS = (_layer(0, 2, 64, 64, True, 0, 'y1', 'p1', 'am1', '_dp1', '_dy1'),
          _layer(1, 5, 64, 128, False, 1, 'p1', 'y5', None, '_dy5', '_dp1'),
          _layer(2, 7, 128, 128, True, 1, 'y5', 'p2', 'am2', '_dp2', '_dy5', own_bias=True))
# the reference's large_cnn (models/asr/transformer.py:60-72): the same arena names -- oracle/branches.py reads them, channel-agnostic
LAYERS_LARGE = (_layer(0, 2, 32, 32, True, 0, 'y1', 'p1', 'am1', '_dp1', '_dy1'),
                _layer(1, 5, 32, 64, False, 1, 'p1', 'y5', None, '_dy5', '_dp1'),
                _layer(2, 7, 64, 64, True, 1, 'y5', 'p2', 'am2', '_dp2', '_dy5', own_bias=True))
STACKS = {'vgg_cnn': LAYERS, 'large_cnn': LAYERS_LARGE}


def layers_for(layout):
    """the layer table of a model, by the output channels of its conv0 (ParamLayout); None: the model has no convolutions
    (feat_extractor='none': the features go straight into the encoder, FrameFront)"""
    if 'conv.0.weight' not in layout.entries:
        return None
    c0 = layout.entries['conv.0.weight'][1][0]
    for layers in STACKS.values():
        if layers[0].cin == c0:
            return layers
    raise NotImplementedError('no convolution stack with %d channels behind conv0' % c0)


def decide(eng, nt, widths):
    """what the front-end of a pass runs on, read ONCE at the start of its forward from the engine's assignable attributes, kept in `saved`.
    A large_cnn model runs on the exact split whatever conv_h2 / conv_x3 say: its 32-channel layers exist in that arithmetic only
    (csrc/mtl_conv_narrow.hip), so conv_mode is 'x3', in_h2 is False and the trainer's periodic h2 census is skipped.  The same holds for a
    model without convolutions (conv_layers None): its input Linear exists on the exact split only (csrc/mtl_featproj.hip)."""
    mode = 'h2' if eng.conv_h2 else ('x3' if eng.conv_x3 else 'f32')
    if eng.conv_layers is not LAYERS:
        mode = 'x3'
    return dict(conv_mode=mode, conv_tb=mode != 'f32' and (nt > 1 or widths is not None), in_h2=mode == 'h2' and eng.in_linear == 'h2')


# The adapters: which call, which argument order.  t: the task of a single-task call, None: all tasks in one `_tb` launch, which takes
# `tail` (the task count and the tasks' strides) behind the single-task arguments.  Call names by [pooled][all tasks] / [all tasks].
class _F32:
    """the fp32-MFMA engine: weights [tap][cin][cout] / [tap][cout][cin] in fp32, no bounds, single-task calls only"""
    WPREP, WGRAD_WS = 'mtl_conv3x3_wprep', 'mtl_conv3x3_wgrad_workspace'
    FWD = (('mtl_conv3x3_relu_fwd',), ('mtl_conv3x3_relu_pool_fwd',))
    DGRAD, WGRAD = ('mtl_conv3x3_dgrad',), ('mtl_conv3x3_wgrad',)
    wshape, wdtype = (), torch.float32

    def weights(self, fr):
        """one wprep per layer and parameter set"""
        for r in fr.layers:
            wf = fr.eng.buf(r.wf, (fr.ntw,) + self.wshape + (9, r.cin, r.cout), self.wdtype)
            wd = fr.eng.buf(r.wd, (fr.ntw,) + self.wshape + (9, r.cout, r.cin), self.wdtype)
            for t in range(fr.ntw):
                check(getattr(fr.lib, self.WPREP)(fr.st, fr.o(r.weight, t), wf[t].data_ptr(), wd[t].data_ptr(), r.cout, r.cin), 'wprep')

    def fwd(self, fr, r, t):
        tb = t is None
        tail = (fr.nt, fr.wstep(r.wf), fr.sP, fr.widths, r.lvl) if tb else ()
        am = (fr.at(r.am, t),) if r.pool else ()
        check(getattr(fr.lib, self.FWD[r.pool][tb])(fr.st, fr.at(r.x, t), fr.at(r.wf, t, fr.wn), fr.o(r.bias, t), fr.at(r.y, t), *am, *fr.dims[r.i],
                                                    *tail), r.y)

    def dgrad(self, fr, r, t):
        tb = t is None
        tail = (fr.nt, fr.wstep(r.wd), fr.widths, r.lvl) if tb else ()
        check(getattr(fr.lib, self.DGRAD[tb])(fr.st, fr.at(r.dy, t), fr.at(r.am, t), fr.at(r.wd, t, fr.wn), fr.at(r.x, t), fr.at(r.dx, t),
                                              *fr.dims[r.i], *tail), r.dx)

    def wgrad(self, fr, r, t, db):
        """db: the bias gradient rides along (sums of dy in the loaders) -- an argument of the several-task launch only, whose partial
        slabs are dealt to the tasks: as many slabs written and reduced as by one single-task launch"""
        tb, am, dims = t is None, fr.at(r.am, t), fr.dims[r.i]
        need = getattr(fr.lib, self.WGRAD_WS)(*dims, 1 if am else 0)
        ride, tail = ((db,), (fr.nt, fr.sG, fr.sG)) if tb else ((), ())
        check(getattr(fr.lib, self.WGRAD[tb])(fr.st, fr.at(r.x, t), fr.at(r.dy, t), am, fr.g(r.weight, t), *ride, fr.eng.scratch(need), need, *dims,
                                              *tail), r.weight)


class _X3(_F32):
    """three exact bf16 pieces of every weight, [piece][tap][cin/32][cout][32] (6 MFMAs per step): fp32's argument order"""
    WPREP, WGRAD_WS = 'mtl_conv3x3_wprep_x3', 'mtl_conv3x3_wgrad_x3_workspace'
    FWD = (('mtl_conv3x3_relu_fwd_x3', 'mtl_conv3x3_relu_fwd_x3_tb'), ('mtl_conv3x3_relu_pool_fwd_x3', 'mtl_conv3x3_relu_pool_fwd_x3_tb'))
    DGRAD, WGRAD = ('mtl_conv3x3_dgrad_x3', 'mtl_conv3x3_dgrad_x3_tb'), ('mtl_conv3x3_wgrad_x3', 'mtl_conv3x3_wgrad_x3_tb')
    wshape, wdtype = (3,), torch.bfloat16


class _H2:
    """two fp16 pieces of every (scaled) operand (3 MFMAs per step): every operand is followed by its bound, every output by the
    slot that receives its bound; per task bitwise the single-task launches (tests/test_ops_gpu.py)"""
    FWD = (('mtl_conv3x3_relu_fwd_h2', 'mtl_conv3x3_relu_fwd_h2_tb'), ('mtl_conv3x3_relu_pool_fwd_h2', 'mtl_conv3x3_relu_pool_fwd_h2_tb'))
    DGRAD, WGRAD = ('mtl_conv3x3_dgrad_h2', 'mtl_conv3x3_dgrad_h2_tb'), ('mtl_conv3x3_wgrad_h2', 'mtl_conv3x3_wgrad_h2_tb')

    def weights(self, fr):
        """all three layers in one call (two launches): of ALL parameter sets when the pass reads a theta' stack"""
        spec, strides = [], []
        for r in fr.layers:
            nb = (fr.lib.mtl_conv3x3_wprep_h2_bytes(r.cout, r.cin) + 255) // 256 * 256       # the pieces + the scale
            wf, wd = fr.eng.buf(r.wf, (fr.ntw, nb), torch.uint8), fr.eng.buf(r.wd, (fr.ntw, nb), torch.uint8)
            spec += [fr.o(r.weight), wf.data_ptr(), wd.data_ptr(), r.cout, r.cin]
            strides.append(wf.stride(0))
        if fr.ntw > 1:
            check(fr.lib.mtl_conv3x3_wprep_h2_batch_tb(fr.st, 3, *spec, fr.ntw, fr.sP, *strides), 'wprep')
        else:
            check(fr.lib.mtl_conv3x3_wprep_h2_batch(fr.st, 3, *spec), 'wprep')

    def fwd(self, fr, r, t):
        tb = t is None      # (the header counts this call's weight stride in elements, the other _tb calls' in bytes: a uint8 buffer, one number)
        tail = (fr.nt, fr.wstep(r.wf), fr.sP, AMAX_STRIDE, AMAX_STRIDE, fr.widths, r.lvl) if tb else ()
        am = (fr.at(r.am, t),) if r.pool else ()
        check(getattr(fr.lib, self.FWD[r.pool][tb])(fr.st, fr.at(r.x, t), fr.am(r.ax, t), fr.at(r.wf, t, fr.wn), fr.o(r.bias, t), fr.at(r.y, t), *am,
                                                    fr.am(r.ay, t), *fr.dims[r.i], *tail), r.y)

    def dgrad(self, fr, r, t):
        """its epilogue delivers the bound of dx, the next layer's bound of dy (conv2: no slot, and bound stride 0 in the _tb call)"""
        tb = t is None
        tail = (fr.nt, fr.wstep(r.wd), AMAX_STRIDE, AMAX_STRIDE if r.adx is not None else 0, fr.widths, r.lvl) if tb else ()
        check(getattr(fr.lib, self.DGRAD[tb])(fr.st, fr.at(r.dy, t), fr.am(r.ady, t), fr.at(r.am, t), fr.at(r.wd, t, fr.wn), fr.at(r.x, t),
                                              fr.at(r.dx, t), fr.am(r.adx, t), *fr.dims[r.i], *tail), r.dx)

    def wgrad(self, fr, r, t, db):
        """db: the bias gradient rides along (the loaders of dy also sum it)"""
        tb, am, dims = t is None, fr.at(r.am, t), fr.dims[r.i]
        need = fr.lib.mtl_conv3x3_wgrad_x3_workspace(*dims, 1 if am else 0)
        tail = (fr.nt, AMAX_STRIDE, AMAX_STRIDE, fr.sG, fr.sG) if tb else ()
        check(getattr(fr.lib, self.WGRAD[tb])(fr.st, fr.at(r.x, t), fr.am(r.ax, t), fr.at(r.dy, t), fr.am(r.ady, t), am, fr.g(r.weight, t), db,
                                              fr.eng.scratch(need), need, *dims, *tail), r.weight)


_ADAPTERS = {'f32': _F32(), 'x3': _X3(), 'h2': _H2()}


class Front:
    """The front-end of one pass in one direction.  S: the pass's record (PassEngine.saved, or what the forward has of it so far):
    theta, x, B, T, F, nt, sP, sX, meta and the three decisions of decide().  Backward: G, sG -- the gradient buffer and its task stride.
    Make it inside the pass and drop it there (see the module's note on eng.lib)."""

    def __init__(self, eng, S, G=None, sG=0):
        self.eng, self.lib, self.st, self.A, self._at = eng, eng.lib, eng.stream, eng.arena, {None: (None, 0)}
        self.nt, self.sP, self.sX, self.B, self.x, self.sG = S['nt'], S['sP'], S['sX'], S['B'], S['x'], sG
        B, T, F = self.B, S['T'], S['F']
        self.TF = TF = ((T, F), (T // 2, F // 2), (T // 2 // 2, F // 2 // 2))  # frames x bins at the three resolution levels
        self.ntw = self.nt if self.sP else 1                                    # distinct parameter sets of this pass
        self.wn = 1 if self.ntw > 1 else 0                                      # rows of a weight buffer from one task to the next
        self.widths, self.mode, self.tb, self.in_h2 = S['meta'].get('widths'), S['conv_mode'], S['conv_tb'], S['in_h2']
        self.tasks = (None,) if self.tb else range(self.nt)
        self.layers = eng.conv_layers
        self.c0, self.c_out = self.layers[0].cin, self.layers[-1].cout         # channels behind conv0 and in front of the input Linear
        self.dims = [(B,) + TF[r.lvl] + (r.cin, r.cout) for r in self.layers]  # by Layer.i
        self.ad = _ADAPTERS[self.mode]
        self.d, self.d_in, self.Me = eng.hp.d, eng.hp.d_in, B * TF[2][0]        # (Me: encoder rows per task)
        # --is-factorized: the input Linear is the pair input_linear_a (d_in -> r, no bias: stage A, the dense Linear's arithmetic at
        # n1 = r outputs) and input_linear_b (r -> d, bias: stage B, an ordinary engine product)
        self.fz = eng.factorized
        self.n1 = eng.hp.r if self.fz else self.d
        self.w_in = 'encoder.input_linear_a.weight' if self.fz else 'encoder.input_linear.weight'
        self.wp_strides = (AMAX_STRIDE, self.n1 * self.d_in) if self.sP else (0, 0)     # bound / weight of the next task's parameter set
        P, sP, off = S['theta'].data_ptr(), self.sP, eng.L.off                   # (no closure below refers to self: a Front is freed with its pass)
        self.o = lambda n, t=None: P + 4 * (off(n) + (t or 0) * sP)             # task t's parameter / its gradient; None: the stack's base
        self.g = lambda n, t=None: G + 4 * (off(n) + (t or 0) * sG)
        if G is None:       # (forward: y1 first, then the bounds -- the order in which the pool has always taken them from the device)
            eng.buf('y1', (self.nt * B, T, F, self.c0))
        amax = (eng.buf('amax', (self.nt, AMAX_PER_TASK, _lib.AMAX_SLOTS)) if G is None else self.A['amax']).data_ptr()
        self.am = (lambda i, t=None: None if i is None else amax + 4 * _lib.AMAX_SLOTS * (AMAX_PER_TASK * (t or 0) + i)) if self.mode == 'h2' \
            else (lambda i, t=None: None)

    def at(self, name, t, n=None):
        """arena buffer `name` (None: no such buffer) at task t; n: its rows per task (the samples; weights: Front.wn); t None: the buffer"""
        e = self._at.get(name)
        if e is None:       # (looked up once per direction: this runs for every pointer of every call of an eagerly enqueued pass)
            b = self.A[name]
            e = self._at[name] = (b.data_ptr(), (self.B if n is None else n) * b.stride(0) * b.element_size())
        return e[0] + t * e[1] if t and e[0] else e[0]

    def wstep(self, name):
        """bytes from one task's prepared weights to the next task's (0: one parameter set)"""
        self.at(name, None, self.wn)
        return self._at[name][1]

    def tails(self, name, lvl, chans):
        """tasks stacked at the widest (prepare_tasks(frames=...)): clear `name` (frames x bins of level lvl x chans floats) beyond every
        task's own frames >> lvl, the zero border of the task's own pass"""
        if self.widths is not None:
            T_, F_ = self.TF[lvl]
            check(self.lib.mtl_zero_tails(self.st, self.at(name, None), self.nt * self.B, T_, F_ * chans, self.widths, lvl, self.B), 'mtl_zero_tails')

    def census(self, names):
        if self.mode == 'h2' and self.eng.census is not None:       # (stream order: every producer has raised its bound by now)
            for n in names:
                slot = SLOT[n.lstrip('_')]
                self.eng._census(slot, self.A[n], self.am(slot))

    # ---- forward
    def convs_fwd(self):
        """x -> y1 -> p1 -> y5 -> p2, and the permuted weight of the input Linear (arena)"""
        eng, nt, B, ad = self.eng, self.nt, self.B, self.ad
        Bt, (T, F) = nt * B, self.TF[0]
        layers = self.layers
        c0 = () if self.c0 == 64 else (self.c0,)        # (64 channels: the calls without a channel count)
        head = (self.st, self.x.data_ptr(), self.o('conv.0.weight'), self.o('conv.0.bias'), self.at('y1', None), B, T, F, *c0, self.am(0))
        if self.mode == 'h2':
            check(self.lib.mtl_memset_zero(self.st, self.am(0), nt * AMAX_STRIDE * 4), 'mtl_memset_zero')
        if nt > 1:      # every task's samples in one launch (task = grid dimension; sX = 0: the shared validation batch), in every mode
            check((self.lib.mtl_conv0c_relu_fwd_tb if c0 else self.lib.mtl_conv0_relu_fwd_tb)(*head, nt, self.sX, self.sP, self.sP, AMAX_STRIDE), 'conv0')
        else:
            check((self.lib.mtl_conv0c_relu_fwd if c0 else self.lib.mtl_conv0_relu_fwd)(*head), 'conv0')
        self.tails('y1', 0, self.c0)
        ad.weights(self)
        for r in layers:
            for name, dtype in ((r.y, torch.float32), (r.am, torch.uint8)):
                if name is not None:
                    eng.buf(name, (Bt,) + self.TF[r.lvl + r.pool] + (r.cout,), dtype)
        if self.tb or self.widths is not None:      # layer by layer; what another convolution reads is cleared before it does
            for r in layers:
                for t in self.tasks:
                    ad.fwd(self, r, t)
                if r is not layers[-1]:
                    self.tails(r.y, r.lvl + r.pool, r.cout)
            if self.tb:     # the launches left out the tile rows beyond a task's frames: everything a later kernel reads there is cleared
                self.tails('p2', 2, self.c_out)         # (after conv7 and with the _tb launches only; the per-task path leaves these three)
                for r in layers:
                    if r.pool:
                        self.tails(r.am, r.lvl + 1, r.cout // 4)      # (arg-max bytes, four to a float)
        else:
            for t in range(nt):                     # task by task
                for r in layers:
                    ad.fwd(self, r, t)
        self.census(('y1', 'p1', 'y5', 'p2'))
        # wp_in: the input Linear's weight with its 5120 (2560) inputs in p2's (bin, channel) order; max|w| rides along; a theta' stack in one launch
        wp = eng.buf('wp_in', (self.ntw, self.n1, self.d_in))
        check(self.lib.mtl_permute_hc_tb(self.st, self.o(self.w_in), wp.data_ptr(), self.n1, self.c_out, self.TF[2][1], 0,
                                         self.am(SLOT['wp']), self.ntw, self.sP, self.n1 * self.d_in, AMAX_STRIDE), 'permute')

    def linear_fwd(self):
        """e0 = p2 . wp^T + b: with the h2 convolutions on two fp16 pieces (one task-batched launch on the tile engine of
        mtl_gemm_x3.hip, per-task bounds by stride), else on the product engines' own routing"""
        eng, nt, Me, d, d_in, (s_am, s_w) = self.eng, self.nt, self.Me, self.d, self.d_in, self.wp_strides
        e0, p2, wp = eng.buf('e0', (nt * Me, d)), self.A['p2'], self.A['wp_in']
        n1, ea = self.n1, (eng.buf('e0a', (nt * Me, self.n1)) if self.fz else e0)      # stage A's output: e0 itself for the dense Linear
        bias = None if self.fz else self.o('encoder.input_linear.bias')
        if self.in_h2:
            check(self.lib.mtl_gemm_h2_tb(self.st, 1, Me, n1, d_in, p2.data_ptr(), d_in, self.am(SLOT['p2']), AMAX_STRIDE, wp.data_ptr(), d_in,
                                          self.am(SLOT['wp']), s_am, ea.data_ptr(), n1, bias, None, 0, nt, Me * d_in,
                                          s_w, Me * n1, self.sP, eng.gemm_ws.data_ptr(), eng.gemm_ws.numel() * 4), 'mtl_gemm_h2_tb')
        else:
            eng.gemm(0, 1, Me, n1, d_in, p2.data_ptr(), d_in, wp.data_ptr(), d_in, ea.data_ptr(), n1, bias=bias,
                     task=(Me * d_in, s_w, Me * n1, self.sP, 0))
        if self.fz:
            eng.linear_fwd(ea.data_ptr(), Me, n1, self.o('encoder.input_linear_b.weight'), self.o('encoder.input_linear_b.bias'), e0.data_ptr(), d)
        return e0

    # ---- backward
    def linear_bwd(self, de0):
        """input_linear.weight += permuted (de0^T . p2); h2: the bound of de0 first (both products of the backward read it)"""
        eng, st, nt, Me, d, d_in = self.eng, self.st, self.nt, self.Me, self.n1, self.d_in
        (T4, F4), p2, a8 = self.TF[2], self.A['p2'], self.am(SLOT['de0'])
        if self.fz:     # stage B first: its weight gradient (the bias came from the input LayerNorm's dsum) and d(e0a), which stage A's two
            dea = eng.buf('_de0a', (nt * Me, d))                    # products then take in de0's place (and in its bound slot); d = r below
            eng.linear_bwd(self.A['e0a'].data_ptr(), de0.data_ptr(), Me, d, self.d, self.o('encoder.input_linear_b.weight'),
                           self.g('encoder.input_linear_b.weight'), None, dea.data_ptr(), False)
            eng.flush_side()
            de0 = dea
        self.de_in = de0
        dwp = eng.buf('_dwp', (nt, d, d_in))
        eng.buf('_dp2', (nt * self.B, T4, F4, self.c_out))
        if self.in_h2:
            if nt > 1:
                check(self.lib.mtl_absmax_f32_tb(st, de0.data_ptr(), Me * d, a8, nt, Me * d, AMAX_STRIDE), 'mtl_absmax_f32')
            else:
                check(self.lib.mtl_absmax_f32(st, de0.data_ptr(), Me * d, a8), 'mtl_absmax_f32')
            eng._census(SLOT['de0'], de0, a8)
            check(self.lib.mtl_gemm_h2_tn_tb(st, d, d_in, Me, de0.data_ptr(), d, a8, AMAX_STRIDE, p2.data_ptr(), d_in, self.am(SLOT['p2']), AMAX_STRIDE,
                                             dwp.data_ptr(), d_in, nt, Me * d, Me * d_in, d * d_in), 'mtl_gemm_h2_tn_tb')
        else:
            eng.gemm(1, 0, d, d_in, Me, de0.data_ptr(), d, p2.data_ptr(), d_in, dwp.data_ptr(), d_in, task=(Me * d, Me * d_in, d * d_in, 0, 0))
        check(self.lib.mtl_permute_hc_tb(st, dwp.data_ptr(), self.g(self.w_in), d, self.c_out, F4, 1, None, nt, d * d_in, self.sG, 0),
              'permute_inv')

    def linear_dgrad(self, de0):
        """dp2 = (de0 . wp) gated by p2 > 0, straight from the un-transposed weight, all tasks in one launch (factorized: d(e0a), which
        linear_bwd formed, against the permuted input_linear_a)"""
        eng, nt, Me, d, d_in, (s_am, s_w) = self.eng, self.nt, self.Me, self.n1, self.d_in, self.wp_strides
        de0 = self.de_in
        p2, wp, dp2 = self.A['p2'], self.A['wp_in'], self.A['_dp2']
        if self.in_h2:
            check(self.lib.mtl_gemm_h2_tb(self.st, 0, Me, d_in, d, de0.data_ptr(), d, self.am(SLOT['de0']), AMAX_STRIDE, wp.data_ptr(), d_in,
                                          self.am(SLOT['wp']), s_am, dp2.data_ptr(), d_in, None, p2.data_ptr(), d_in, nt, Me * d, s_w, Me * d_in, 0,
                                          None, 0), 'mtl_gemm_h2_tb')
        else:
            eng.gemm(0, 0, Me, d_in, d, de0.data_ptr(), d, wp.data_ptr(), d_in, dp2.data_ptr(), d_in, gate=p2.data_ptr(), ldg=d_in,
                     task=(Me * d, s_w, Me * d_in, 0, 0))

    def convs_bwd(self):
        """dp2 -> the parameter gradients of conv7, conv5, conv2 and conv0"""
        eng, lib, st, nt, B, ad, layers = self.eng, self.lib, self.st, self.nt, self.B, self.ad, self.layers
        T, F = self.TF[0]
        c0 = () if self.c0 == 64 else (self.c0,)
        for r in layers[::-1]:
            eng.buf(r.dx, (nt * B,) + self.TF[r.lvl] + (r.cin,))
        # the bias gradients of conv5 / conv2 ride on their weight-gradient launches: always with h2 (the data-gradient epilogues also
        # deliver the next bound, so the column-sum passes over dy5 and dp1 are not needed), with the exact split in the several-task launches
        ride = self.mode == 'h2' or self.tb
        for t in self.tasks:
            for r in layers[::-1]:
                To, Fo = self.TF[r.lvl + r.pool]
                bias, own = self.g(r.bias, t), r.own_bias or not ride
                if own and t is None:
                    per = ((lib.mtl_colsum_workspace(B * To * Fo, r.cout) // 4 + 3) // 4 * 4) * 4
                    check(lib.mtl_colsum_accum_tb(st, self.at(r.dy, t), B * To * Fo, r.cout, bias, eng.scratch(nt * per + 64), self.am(r.ady), nt,
                                                  self.sG, AMAX_STRIDE), 'colsum_tb')
                elif own:
                    eng.colsum(self.at(r.dy, t), B * To * Fo, r.cout, bias, self.am(r.ady, t))
                ad.wgrad(self, r, t, None if own else bias)
                ad.dgrad(self, r, t)
                if self.tb:     # the launch left out the tile rows beyond a task's frames: bias sums, bounds and weight gradients read whole tensors
                    self.tails(r.dx, r.lvl, r.cin)
            head = (st, self.x.data_ptr() + 4 * (t or 0) * self.sX, self.at('_dy1', t), self.g('conv.0.weight', t), self.g('conv.0.bias', t),
                    eng.scratch(lib.mtl_conv0_wgrad_workspace()), B, T, F, *c0)
            if t is None:
                check((lib.mtl_conv0c_wgrad_tb if c0 else lib.mtl_conv0_wgrad_tb)(*head, nt, self.sX, self.sG, self.sG), 'wgrad0_tb')
            else:
                check((lib.mtl_conv0c_wgrad if c0 else lib.mtl_conv0_wgrad)(*head), 'wgrad0')
        self.census(('_dp2', '_dy5', '_dp1'))


class FrameFront:
    """The front of a model WITHOUT convolutions (feat_extractor='none', models/asr/transformer.py:93-94: the (B, 1, F, T) batch viewed as
    (B, F, T) and transposed; modules/encoder.py: Linear(F -> d) on every frame), with Front's five methods.  There is nothing to
    convolve and no data gradient (the features carry none); the input Linear and its weight gradient run on the feature planes as the
    batch brings them and the weight as theta holds it (csrc/mtl_featproj.hip: no transposed or padded copy of either), all tasks of
    the pass in one launch.  Every frame is an encoder position: tasks stacked at the widest bring zero frames beyond their own width
    (the batch builder pads with zeros), whose rows come out as the bias and are masked like any padding (batchmeta: klen_enc, keep_enc).
    --is-factorized: stage A (input_linear_a, r x F, no bias) is the same kernel at N = r; stage B and its backward are Front's."""

    def __init__(self, eng, S, G=None, sG=0):
        self.eng, self.lib, self.st, self.A = eng, eng.lib, eng.stream, eng.arena
        self.nt, self.sP, self.sX, self.B, self.x, self.sG = S['nt'], S['sP'], S['sX'], S['B'], S['x'], sG
        self.T, self.F = S['T'], S['F']
        self.d, self.Me = eng.hp.d, self.B * self.T                             # (Me: encoder rows per task)
        self.fz = eng.factorized
        self.n1 = eng.hp.r if self.fz else self.d
        self.w_in = 'encoder.input_linear_a.weight' if self.fz else 'encoder.input_linear.weight'
        P, sP, off = S['theta'].data_ptr(), self.sP, eng.L.off
        self.o = lambda n: P + 4 * off(n)                                       # (the stack's base: the launches stride the tasks)
        self.g = lambda n: G + 4 * off(n)

    def convs_fwd(self):
        pass

    def linear_fwd(self):
        """e0 = x^T . w^T + b for every frame of every task"""
        eng, nt, Me, d, n1 = self.eng, self.nt, self.Me, self.d, self.n1
        e0 = eng.buf('e0', (nt * Me, d))
        ea = eng.buf('e0a', (nt * Me, n1)) if self.fz else e0
        bias = None if self.fz else self.o('encoder.input_linear.bias')
        check(self.lib.mtl_featproj_fwd_tb(self.st, self.x.data_ptr(), self.o(self.w_in), bias, ea.data_ptr(), self.B, self.F, self.T, n1, nt,
                                           self.sX, self.sP, Me * n1), 'mtl_featproj_fwd_tb')
        if self.fz:
            eng.linear_fwd(ea.data_ptr(), Me, n1, self.o('encoder.input_linear_b.weight'), self.o('encoder.input_linear_b.bias'), e0.data_ptr(), d)
        return e0

    def linear_bwd(self, de0):
        """input_linear.weight += de0^T . x^T (the bias came from the input LayerNorm's dsum); factorized: stage B's weight gradient and
        d(e0a) first, as in Front.linear_bwd"""
        eng, nt, Me, n1 = self.eng, self.nt, self.Me, self.n1
        if self.fz:
            dea = eng.buf('_de0a', (nt * Me, n1))
            eng.linear_bwd(self.A['e0a'].data_ptr(), de0.data_ptr(), Me, n1, self.d, self.o('encoder.input_linear_b.weight'),
                           self.g('encoder.input_linear_b.weight'), None, dea.data_ptr(), False)
            eng.flush_side()
            de0 = dea
        need = self.lib.mtl_featproj_wgrad_workspace(self.B, self.F, self.T, n1, nt)
        check(self.lib.mtl_featproj_wgrad_tb(self.st, self.x.data_ptr(), de0.data_ptr(), self.g(self.w_in), eng.scratch(need), need, self.B,
                                             self.F, self.T, n1, nt, self.sX, Me * n1, self.sG), 'mtl_featproj_wgrad_tb')

    def linear_dgrad(self, de0):
        pass

    def convs_bwd(self):
        pass


def front_for(eng, S, G=None, sG=0):
    """the front of a pass in one direction: the conv stack's (Front) or, for a model without convolutions, FrameFront"""
    return (FrameFront if eng.conv_layers is None else Front)(eng, S, G, sG)


def time_shift(layout):
    """log2 of the front-end's time reduction (batchmeta.enc_extent): two max-pools behind either conv stack, none without one"""
    return CONV_TIME_SHIFT if 'conv.0.weight' in layout.entries else 0
