"""The layout of the ctypes front: HipOps is composed from one class per mission (ops_base, ops_window, ops_seg, ops_prep)
and holds the calibration wrappers itself.  Importing the modules needs no device."""
import inspect

from efficientq_amd import hip_ops, ops_base, ops_prep, ops_seg, ops_window
from efficientq_amd.hip_ops import HipOps
from efficientq_amd.ops_base import OpsBase
from efficientq_amd.ops_prep import PrepOps
from efficientq_amd.ops_seg import SegOps
from efficientq_amd.ops_window import WindowOps

CLASSES = (OpsBase, WindowOps, SegOps, PrepOps, HipOps)
REEXPORTS = ("HipOps", "get_ops", "make_geom", "to_ndhwc", "from_ndhwc", "_ptr", "check", "ADMM_TOL", "FP_BRACKET_MIN",
             "BLEND_KINDS", "blend_weights_host", "conv_plan_query", "conv_i8_plan_query", "conv_i8s_plan_query",
             "CONV_KINDS", "CONV_I8_KERNELS")

# every non-dunder attribute of HipOps with the signature of the callables, as the class stood before it was split
# (str(inspect.signature(getattr(HipOps, name))); None: a property or a constant)
SURFACE = [
    ('GRAM_I8_MAX_CLASSES', None),
    ('PROX_SHIFT_TERMS', None),
    ('_admm_read_channels', '(run, best, err, extra)'),
    ('_axis_weights', "(what: 'str', spacing)"),
    ('_elsewhere', "(self, t: 'torch.Tensor') -> 'bool'"),
    ('_f32', "(self, t: 'torch.Tensor') -> 'torch.Tensor'"),
    ('_fit_scale_bracket', '(self, x, n, levels, lo, hi, reducer, batch, st, s0, cap)'),
    ('_fit_scale_gathered', '(self, x, n, levels, lo, hi, reducer, st, ws, cap)'),
    ('_fuse_code', "(what: 'str', fuse, argmax: 'bool', by: 'str', Cc: 'int', rule: 'Optional[str]' = None) -> 'int'"),
    ('_mask_planes', "(self, what: 'str', mask: 'torch.Tensor')"),
    ('_orient_plan', "(what: 'str', src_axis, flip)"),
    ('_prep_box', "(what: 'str', shape, pmin, pmax)"),
    ('_prep_mask', "(what: 'str', mask: 'str') -> 'int'"),
    ('_prep_stats', "(self, what: 'str', v, n: 'int') -> 'torch.Tensor'"),
    ('_prep_volumes', "(self, what: 'str', x: 'torch.Tensor', dtype=torch.float32, limit_c: 'bool' = True)"),
    ('_seg_case', "(self, what: 'str', logits: 'torch.Tensor', label: 'torch.Tensor', task: 'str', fuse, spatial: 'bool')"),
    ('_table_call', "(self, what: 'str', P: 'int', head: 'int', width: 'int', max_rows, call)"),
    ('_window_case', '(self, shape, patch, overlap)'),
    ('_window_channels', "(what: 'str', Cc: 'int')"),
    ('_workspace', "(self, key: 'str', nbytes: 'int') -> 'torch.Tensor'"),
    ('abs_sum', "(self, x: 'torch.Tensor') -> 'torch.Tensor'"),
    ('act_quant_backward', "(self, x: 'torch.Tensor', alpha: 'torch.Tensor', levels: 'int', gq: 'torch.Tensor', want_gx=True)"),
    ('adam_step', "(self, p, g, m, v, lr: 'float', t: 'int', b1=0.9, b2=0.999, eps=1e-08)"),
    ('admm_presum', '(self, wstar, dual, v)'),
    ('admm_project_dual', "(self, v, wstar, state, levels: 'int', G, dual, dual_div: 'float', Gq=None)"),
    ('admm_read', '(run, best, extra=None)'),
    ('admm_run', "(self, A0, B0, W0, b0, geom: 'Geom', y_ndhwc, *, xq=None, xidx=None, act_alpha=None, act_levels: 'int' = 0, loss_kind: 'int' = 0, rho: 'float', rho_max: 'float', eta: 'float', iters: 'int', period: 'int', levels: 'int', overlap: 'bool' = True, loss_gram=None, residuals: 'bool' = False, channel_wise: 'bool' = False)"),
    ('admm_select_best', '(self, run)'),
    ('att_classes', "(self, att: 'Optional[torch.Tensor]')"),
    ('blend_weights', "(self, patch, kind: 'str' = 'uniform')"),
    ('cc_label', "(self, mask: 'torch.Tensor', connectivity: 'int' = 26)"),
    ('cc_table', "(self, mask: 'torch.Tensor', connectivity: 'int' = 26, max_rows: 'Optional[int]' = None)"),
    ('channel_alpha_best', '(run, best)'),
    ('conv_forward_i8', "(self, xidx: 'torch.Tensor', G: 'torch.Tensor', bias, geom: 'Geom', y_ndhwc: 'torch.Tensor', att, act_alpha: 'torch.Tensor', act_levels: 'int', w_state: 'torch.Tensor', w_levels: 'int')"),
    ('conv_i8_out_supported', "(self, geom: 'Geom', act_levels: 'int', w_levels: 'int') -> 'bool'"),
    ('conv_i8_plan', "(self, geom: 'Geom', want_out: 'bool' = False) -> 'dict'"),
    ('conv_i8_supported', "(self, geom: 'Geom', act_levels: 'int', w_levels: 'int') -> 'bool'"),
    ('conv_i8s_plan', "(self, geom: 'Geom', act_levels: 'int', w_levels: 'int') -> 'dict'"),
    ('conv_i8s_supported', "(self, geom: 'Geom', act_levels: 'int', w_levels: 'int') -> 'bool'"),
    ('conv_plan', "(self, geom: 'Geom', loss_only: 'bool' = False) -> 'dict'"),
    ('conv_step', "(self, x_ndhwc: 'torch.Tensor', weight: 'torch.Tensor', bias: 'Optional[torch.Tensor]', geom: 'Geom', y_ndhwc: 'Optional[torch.Tensor]' = None, att: 'Optional[torch.Tensor]' = None, act_alpha: 'Optional[torch.Tensor]' = None, act_levels: 'int' = 0, want_out: 'bool' = False, sqerr: 'Optional[torch.Tensor]' = None)"),
    ('conv_step_i8', "(self, xidx: 'torch.Tensor', Gq: 'torch.Tensor', bias, geom: 'Geom', y_ndhwc: 'torch.Tensor', act_alpha: 'torch.Tensor', act_levels: 'int', w_state: 'torch.Tensor', w_levels: 'int', sqerr)"),
    ('conv_step_i8s', "(self, xidx: 'torch.Tensor', Gq: 'torch.Tensor', bias, geom: 'Geom', y_ndhwc: 'torch.Tensor', act_alpha: 'torch.Tensor', act_levels: 'int', w_state: 'torch.Tensor', w_levels: 'int', sqerr, prepare: 'bool')"),
    ('default_sigmoid_threshold', "(self) -> 'float'"),
    ('edt_sq', "(self, mask: 'torch.Tensor')"),
    ('edt_sq_mm', "(self, mask: 'torch.Tensor', spacing)"),
    ('fit_scale', "(self, x: 'torch.Tensor', levels: 'int', lo: 'float', hi: 'float', reducer=None, guess_iters: 'int' = 16, state: 'Optional[torch.Tensor]' = None, abs_sums: 'Optional[torch.Tensor]' = None)"),
    ('fixed_point_bucket', "(self, a, b, v, levels: 'int', state, lo: 'float' = -1.0, hi: 'float' = 1.0)"),
    ('fixed_point_bucket_rec', "(self, a, b, v, levels: 'int', state, pred, lo: 'float' = -1.0, hi: 'float' = 1.0)"),
    ('fixed_point_channels', "(self, a, b, v, levels: 'int', alpha, iters=None, err_flag=None, proj=None)"),
    ('fixed_point_coop_rec', "(self, a, b, v, levels: 'int', state, pred, lo: 'float' = -1.0, hi: 'float' = 1.0)"),
    ('fixed_point_traj', "(self, a, b, v, levels: 'int', state, pred, lo: 'float' = -1.0, hi: 'float' = 1.0)"),
    ('fp_bracket_diagnostics', '(self)'),
    ('fp_check', '(self, state, err_flag)'),
    ('gram', "(self, x_ndhwc: 'torch.Tensor', att: 'Optional[torch.Tensor]', y_ndhwc: 'torch.Tensor', geom: 'Geom', has_bias: 'bool', A0: 'Optional[torch.Tensor]' = None, B0: 'Optional[torch.Tensor]' = None)"),
    ('gram_f64', "(self, x_ndhwc: 'torch.Tensor', y_ndhwc: 'torch.Tensor', geom: 'Geom', has_bias: 'bool')"),
    ('gram_f64_pipelined', "(self, x_ndhwc: 'torch.Tensor', y_ndhwc: 'torch.Tensor', geom: 'Geom', has_bias: 'bool') -> 'bool'"),
    ('gram_f64_plan', "(self, geom: 'Geom', has_bias: 'bool') -> 'dict'"),
    ('gram_f64_supported', "(self, geom: 'Geom', has_bias: 'bool') -> 'bool'"),
    ('gram_i8', "(self, xidx_ndhwc: 'torch.Tensor', att_cls, y_ndhwc: 'torch.Tensor', geom: 'Geom', has_bias: 'bool', act_alpha: 'torch.Tensor', act_levels: 'int', A0: 'Optional[torch.Tensor]' = None, B0: 'Optional[torch.Tensor]' = None, unweighted: 'bool' = False)"),
    ('gram_i8_groups', "(self, geom: 'Geom', ncls: 'int' = 1, n_list: 'int' = 0) -> 'dict'"),
    ('gram_i8_plan', "(self, geom: 'Geom', ncls: 'int' = 1, n_list: 'int' = 0) -> 'dict'"),
    ('gram_i8_set_group', "(self, gi: 'int', gj: 'int') -> 'None'"),
    ('gram_i8_supported', "(self, geom: 'Geom', act_levels: 'int') -> 'bool'"),
    ('gram_loss', "(self, Au: 'torch.Tensor', Bu: 'torch.Tensor', syy: 'torch.Tensor', G: 'torch.Tensor', b, sqerr=None)"),
    ('gram_loss_i8', "(self, planes, Au, Bu, syy, Gq, b, states, act_alpha, act_levels: 'int', w_levels: 'int', hist=None)"),
    ('gram_loss_i8_planes', "(self, Au: 'torch.Tensor', has_b: 'bool', act_alpha: 'torch.Tensor', act_levels: 'int', voxels: 'int')"),
    ('gram_loss_i8_supported', "(self, c2: 'int', n: 'int', has_b: 'bool', w_levels: 'int') -> 'bool'"),
    ('gram_plan', "(self, geom: 'Geom', has_bias: 'bool') -> 'dict'"),
    ('gram_reduce', "(self, A0: 'torch.Tensor', B0: 'torch.Tensor', reducer)"),
    ('gram_streamed', "(self, x_ndhwc: 'torch.Tensor', y_ndhwc: 'torch.Tensor', geom: 'Geom', has_bias: 'bool') -> 'bool'"),
    ('label_clean', "(self, label_map: 'torch.Tensor', rules, connectivity: 'int' = 26, out: 'Optional[torch.Tensor]' = None)"),
    ('label_tallies', "(self, pred: 'torch.Tensor', truth: 'torch.Tensor', lut, C_: 'int')"),
    ('loss_stream', '(self)'),
    ('moments', "(self, x: 'torch.Tensor') -> 'torch.Tensor'"),
    ('new_fp_pred', "(self) -> 'torch.Tensor'"),
    ('new_fp_state', "(self) -> 'torch.Tensor'"),
    ('pack_levels', "(self, idx: 'torch.Tensor', bits: 'int') -> 'torch.Tensor'"),
    ('prep_bbox_moments', "(self, x: 'torch.Tensor', mask: 'str' = 'nonzero')"),
    ('prep_crop_u8', "(self, x: 'torch.Tensor', pmin, pmax) -> 'torch.Tensor'"),
    ('prep_cubic_plan', "(self, shape, out_shape) -> 'dict'"),
    ('prep_quantiles', "(self, x: 'torch.Tensor', qs, mask: 'str' = 'nonzero')"),
    ('prep_reorient', "(self, x: 'torch.Tensor', src_axis, flip) -> 'torch.Tensor'"),
    ('prep_reorient_variant', "(self, src_axis, flip, elem_bytes: 'int') -> 'int'"),
    ('prep_resample', "(self, x: 'torch.Tensor', factors, out_shape, nearest: 'bool' = False) -> 'torch.Tensor'"),
    ('prep_resample_cubic', "(self, x: 'torch.Tensor', factors, out_shape, keep_zero: 'bool' = False) -> 'torch.Tensor'"),
    ('prep_smooth', "(self, x: 'torch.Tensor', sigmas, keep_zero: 'bool' = False) -> 'torch.Tensor'"),
    ('prep_spline_prefilter', "(self, x: 'torch.Tensor', passes: 'str' = 'dhw', out: 'Optional[torch.Tensor]' = None)"),
    ('prep_sqdev', "(self, x: 'torch.Tensor', mean, mask: 'str' = 'nonzero') -> 'torch.Tensor'"),
    ('prep_standardise_crop', "(self, x: 'torch.Tensor', pmin, pmax, mean, std, mask: 'str' = 'nonzero') -> 'torch.Tensor'"),
    ('prep_union_mask', "(self, x: 'torch.Tensor', mask: 'str' = 'nonzero') -> 'torch.Tensor'"),
    ('prep_window', "(self, x: 'torch.Tensor', lo: 'float', hi: 'float') -> 'torch.Tensor'"),
    ('prep_window_mask', "(self, x: 'torch.Tensor', lo: 'float', hi: 'float', mask: 'str' = 'nonzero') -> 'torch.Tensor'"),
    ('prox_plan', "(self, c2: 'int', n: 'int') -> 'dict'"),
    ('prox_solve', "(self, B0, Ainv, W0, b0, G, dual, rho: 'float', eta: 'float', wstar, bstar)"),
    ('prox_solve_shifted', "(self, B0, Ainv, W0, b0, G, dual, rho: 'float', eta: 'float', rho_inv: 'float', wstar, bstar)"),
    ('quant_dequant_f32', "(self, x: 'torch.Tensor', alpha: 'torch.Tensor', levels: 'int', lo: 'float', hi: 'float', want_idx: 'bool' = False)"),
    ('quant_dequant_f64path', "(self, x: 'torch.Tensor', state: 'torch.Tensor', levels: 'int', lo: 'float', hi: 'float', want_b: 'bool' = False, want_idx: 'bool' = False)"),
    ('read_fp_pred', "(pred: 'torch.Tensor')"),
    ('read_fp_state', "(state: 'torch.Tensor')"),
    ('release_retired', '(self)'),
    ('seg_agreement', "(self, logits_q: 'torch.Tensor', logits_fp: 'torch.Tensor', mode: 'str', fuse: 'Optional[str]' = None, want_map: 'bool' = False)"),
    ('seg_labels', "(self, logits: 'torch.Tensor', rule: 'str', fuse: 'Optional[str]' = None, dtype=torch.uint8)"),
    ('seg_labels_source', "(self, logits: 'torch.Tensor', pmin, grid, factors, source_shape, rule: 'str', fuse: 'Optional[str]' = None) -> 'torch.Tensor'"),
    ('seg_lesion_table', "(self, logits: 'torch.Tensor', label: 'torch.Tensor', task: 'str', fuse: 'Optional[str]' = None, max_rows: 'Optional[int]' = None)"),
    ('seg_lesions', "(self, logits: 'torch.Tensor', label: 'torch.Tensor', task: 'str', fuse: 'Optional[str]' = None)"),
    ('seg_probs_source', "(self, logits: 'torch.Tensor', pmin, grid, factors, source_shape, mode: 'str', want_prob: 'bool' = True, want_unc: 'bool' = False)"),
    ('seg_surface', "(self, logits: 'torch.Tensor', label: 'torch.Tensor', task: 'str', fuse: 'Optional[str]' = None)"),
    ('seg_surface_mm', "(self, logits: 'torch.Tensor', label: 'torch.Tensor', task: 'str', fuse: 'Optional[str]' = None, spacing=(1.0, 1.0, 1.0))"),
    ('seg_sweep', "(self, logits: 'torch.Tensor', label: 'torch.Tensor', task: 'str', fuse: 'Optional[str]' = None)"),
    ('seg_sweep_plan', "(self, Cc: 'int', S: 'int', task: 'str') -> 'dict'"),
    ('seg_tallies', "(self, logits: 'torch.Tensor', label: 'torch.Tensor', task: 'str', fuse: 'Optional[str]' = None)"),
    ('set_decision_threshold', "(self, logit: 'Optional[float]') -> 'None'"),
    ('shift_terms', "(self, rho: 'float', eta: 'float', rho_inv: 'float') -> 'int'"),
    ('side_stream', '(self)'),
    ('side_stream2', '(self)'),
    ('sigmoid_threshold', "(self) -> 'float'"),
    ('spd_inverse', "(self, A0: 'torch.Tensor', has_bias: 'bool', rho: 'float', eta: 'float', out: 'Optional[torch.Tensor]' = None, ws_key: 'str' = 'inv') -> 'torch.Tensor'"),
    ('spd_inverse_plan', "(self, n: 'int') -> 'dict'"),
    ('storage_bits', "(levels: 'int') -> 'int'"),
    ('stream', None),
    ('sweep_edges', "(self, kind: 'str') -> 'torch.Tensor'"),
    ('unpack_levels', "(self, packed: 'torch.Tensor', n: 'int', bits: 'int') -> 'torch.Tensor'"),
    ('upsample_trilinear', "(self, x_ndhwc: 'torch.Tensor', scale) -> 'torch.Tensor'"),
    ('warm_streams', '(self)'),
    ('weight_fixed_point', "(self, wstar, dual, v, levels: 'int', state, guess: 'int' = 16)"),
    ('window_gather', "(self, vol: 'torch.Tensor', patch, overlap, first: 'int' = 0, count: 'Optional[int]' = None, flip: 'int' = 0)"),
    ('window_grid', "(dhw, patch, overlap) -> 'Tuple[int, int, int]'"),
    ('window_put', "(self, last: 'torch.Tensor', buf_slice: 'torch.Tensor', flip: 'int' = 0, accumulate: 'bool' = False) -> 'None'"),
    ('window_stitch', "(self, win: 'torch.Tensor', shape, patch, overlap, weights=None, nflip: 'int' = 1) -> 'torch.Tensor'"),
]


def test_no_name_is_defined_by_two_classes():
    """A helper of the same name in two mixins (or in a mixin and HipOps) would be shadowed silently by the MRO."""
    owner = {}
    for cls in CLASSES:
        for name in vars(cls):
            if name.startswith("__") and name.endswith("__"):
                continue
            assert name not in owner, f"{name} is defined by {owner[name].__name__} and by {cls.__name__}"
            owner[name] = cls
    assert HipOps.__mro__[:5] == (HipOps, WindowOps, SegOps, PrepOps, OpsBase)


def test_hip_ops_keeps_every_name_that_is_imported_from_it():
    missing = [n for n in REEXPORTS if not hasattr(hip_ops, n)]
    assert not missing, missing
    assert hip_ops.HipOps is HipOps and hip_ops.BLEND_KINDS is ops_window.BLEND_KINDS
    assert hip_ops.blend_weights_host is ops_window.blend_weights_host and hip_ops._ptr is ops_base._ptr


def test_the_patched_constants_live_in_hip_ops_alone():
    """Tests assign to hip_ops.ADMM_TOL and hip_ops.FP_BRACKET_MIN; a copy in another module would not follow them."""
    for mod in (ops_base, ops_window, ops_seg, ops_prep):
        for name in ("ADMM_TOL", "FP_BRACKET_MIN"):
            assert not hasattr(mod, name), f"{mod.__name__}.{name}"


def test_public_surface_is_what_it_was_before_the_split():
    got = []
    for name in dir(HipOps):
        if name.startswith("__"):
            continue
        attr = getattr(HipOps, name)
        got.append((name, str(inspect.signature(attr)) if callable(attr) else None))
    assert got == SURFACE, sorted(set(got) ^ set(SURFACE))
    assert isinstance(inspect.getattr_static(HipOps, "window_grid"), staticmethod)
    assert HipOps.window_grid((8, 8, 8), 4, 2) == (3, 3, 3)
