"""Device operators: torch tensors in, torch tensors out, computed by libidgrec.so's HIP
kernels through the C ABI.  PyTorch only supplies device memory, streams and autograd
bookkeeping.  Every operator requires CUDA(=HIP) tensors; there is no CPU implementation —
calling one with CPU tensors raises.

Operator boundary: `spmm(graph, X)` stands where the reference calls
`torch.sparse.mm(self.Graph, X)` (models/LightGCN.py:44); `propagate_mean` is the whole
`aggregate()` loop (models/LightGCN.py:36-52); `bpr_loss` is the gather + get_bpr_loss +
reg_lambda*get_reg_loss of `forward()` (models/LightGCN.py:57-68); `score_topk` is
get_rating_for_test + mask + torch.topk (utility/utility_train/batch_test.py:59-68).

A package by kernel family (a <- b: b imports a): _base (helpers, LocalEvent, the workspace cache) <- graph (idg_graph and
the families every encoder builds on, each under its header: ssl, rownorm, bpr, dense / ngcf, gccf, gcmc, group, intent,
hyper) <- vae; on _base alone, one module per csrc/idg_*.hip unit and named after it: au, sccf, nance, tnce, mixnce,
svdnce, kmeans, adam, score.  No module imports this package; every name, private ones included, is re-exported here, and
module state (the noise stream, `_compose_views`, every workspace cache) is one object, mutated and never rebound.
"""
from ..native import check, lib  # noqa: F401
from ._base import (  # noqa: F401
    LocalEvent, _cached_ws, _f32c, _i64c, _ld, _ptr, _raw_stream, _require_device, _require_ids, _row_base, _stream, side_stream,
)
from .adam import Adam, adam_step_raw
from .au import (  # noqa: F401
    _AlignUniform, _AlignUniformSame, _au_ws_cache, align_uniform_loss, align_uniform_raw, align_uniform_workspace,
)
from .graph import (  # noqa: F401
    GCMC_SLOPE, GROUP_MAX, Graph, GroupCsr, IMPGCN_DROP, IMPGCN_SLOPE, ROWNORM_EPS, ROWNORM_MAX_WIDTH, SSL_CROSS, SSL_RAW,
    SSL_UNIQUE, _BprLoss, _BprLossSame, _EncodeRows, _GccfLayer, _GcmcLayer, _GroupedPropagate, _HyperMix, _InfoNCEPair,
    _IntentMix, _NgcfTail, _NgcfTransform, _PropagateMean, _PropagateNormalized, _PropagateViews, _RowsNormalize, _SpMM,
    _SpMMNoise, _TallLinear, _bpr_ws, _bpr_ws_cache, _check_groups, _check_member, _colsum_ws, _compose_views,
    _forget_units_of, _forget_units_ws, _gccf_ws, _gcmc_ws, _hyper_rows, _hyper_workspace, _hyper_ws, _intent_ws, _mask_base,
    _next_noise_stream, _noise_stream, _rownorm_args, _ssl_ws, _wgrad_ws, bitmap_clear_raw, bpr_fused_raw, bpr_fwd_bwd_raw,
    bpr_loss, bpr_pack_rows_raw, bpr_plan_raw, bpr_rows_message_floats, bpr_touch_rows_raw, bpr_unpack_rows_raw,
    bpr_workspace, colsum_raw, encode_rows, flags_compact_raw, gccf_layer, gccf_layer_bwd_raw, gccf_layer_fwd_raw, gcmc_layer,
    gcmc_layer_bwd_raw, gcmc_layer_fwd_raw, grad_tail_adam_raw, group_assign_raw, group_grad_raw, grouped_propagate,
    grouped_spmm_raw, hyper_bwd_raw, hyper_close_raw, hyper_expand_raw, hyper_latent_raw, hyper_mix, infonce_cross_raw,
    infonce_pair, infonce_pair_raw, infonce_plan_raw, infonce_workspace, intent_bwd_raw, intent_fwd_raw, intent_mix,
    intent_noise_raw, layer_noise_stream, lincomb_raw, linear_wgrad_raw, ngcf_layer_tail, ngcf_transform, perturb_raw,
    propagate_mean, propagate_normalized, propagate_views, propagate_views_raw, reset_noise_stream, rows_chain_add_raw,
    rows_chain_store2_raw, rows_gather2_raw, rows_gather_raw, rows_layer_mean_raw, rows_normalize, rows_normalize_bwd_raw,
    rows_normalize_raw, rows_scatter_raw, rows_tanh_bwd_raw, spmm, spmm_epi_raw, spmm_ex_raw, spmm_noise_raw, spmm_perturbed,
    spmm_rows_width, subgraph_values_raw, tall_linear, users_bitmap,
)
from .kmeans import (  # noqa: F401
    KMEANS_MAX_WIDTH, _kmeans_args, _kmeans_ws_cache, kmeans, kmeans_assign_raw, kmeans_raw, kmeans_update_raw,
    kmeans_workspace,
)
from .mixnce import MIX_NCE_MAX_WIDTH, _MixNCE, _mix_ws_cache, mix_nce, mix_nce_raw, mix_nce_workspace  # noqa: F401
from .nance import (  # noqa: F401
    _NaNceLoss, _RegRows, _na_ws, _na_ws_cache, na_nce_loss, na_nce_loss_raw, na_nce_workspace, reg_rows_loss, reg_rows_raw,
)
from .sccf import _SCCFLoss, _sccf_ws_cache, sccf_loss, sccf_loss_raw, sccf_workspace  # noqa: F401
from .score import score_dense, score_topk, score_topk_form, topk_option, topk_options
from .svdnce import (  # noqa: F401
    LOWRANK_MAX_RANK, SVD_NCE_MAX_WIDTH, _LowrankExpand, _LowrankProject, _SvdNCE, _lowrank_rows, _lowrank_sizes,
    _lowrank_ws_cache, _rows_panel, _svd_nce_args, _svd_nce_ws_cache, lowrank_expand, lowrank_expand_raw, lowrank_project,
    lowrank_project_raw, svd_nce_loss, svd_nce_raw, svd_nce_workspace,
)
from .tnce import (  # noqa: F401
    TABLE_NCE_MAX_WIDTH, _TableNCE, _table_nce_args, _tnce_ws_cache, table_nce_loss, table_nce_raw, table_nce_workspace,
)
from .vae import (  # noqa: F401
    _MultinomialNLL, _VaeHead, _head_args, _head_workspace, _head_ws, multinomial_nll, multinomial_nll_raw,
    multinomial_nll_workspace, vae_head, vae_head_bwd_raw, vae_head_raw,
)

__all__ = [
    "Adam", "GCMC_SLOPE", "GROUP_MAX", "Graph", "GroupCsr", "IMPGCN_DROP", "IMPGCN_SLOPE", "KMEANS_MAX_WIDTH",
    "LOWRANK_MAX_RANK", "LocalEvent", "MIX_NCE_MAX_WIDTH", "ROWNORM_EPS", "ROWNORM_MAX_WIDTH", "SSL_CROSS", "SSL_RAW",
    "SSL_UNIQUE", "SVD_NCE_MAX_WIDTH", "TABLE_NCE_MAX_WIDTH", "adam_step_raw", "align_uniform_loss", "align_uniform_raw",
    "align_uniform_workspace", "bitmap_clear_raw", "bpr_fused_raw", "bpr_fwd_bwd_raw", "bpr_loss", "bpr_pack_rows_raw",
    "bpr_plan_raw", "bpr_rows_message_floats", "bpr_touch_rows_raw", "bpr_unpack_rows_raw", "bpr_workspace", "colsum_raw",
    "encode_rows", "flags_compact_raw", "gccf_layer", "gccf_layer_bwd_raw", "gccf_layer_fwd_raw", "gcmc_layer",
    "gcmc_layer_bwd_raw", "gcmc_layer_fwd_raw", "grad_tail_adam_raw", "group_assign_raw", "group_grad_raw",
    "grouped_propagate", "grouped_spmm_raw", "hyper_bwd_raw", "hyper_close_raw", "hyper_expand_raw", "hyper_latent_raw",
    "hyper_mix", "infonce_cross_raw", "infonce_pair", "infonce_pair_raw", "infonce_plan_raw", "infonce_workspace",
    "intent_bwd_raw", "intent_fwd_raw", "intent_mix", "intent_noise_raw", "kmeans", "kmeans_assign_raw", "kmeans_raw",
    "kmeans_update_raw", "kmeans_workspace", "layer_noise_stream", "lincomb_raw", "linear_wgrad_raw", "lowrank_expand",
    "lowrank_expand_raw", "lowrank_project", "lowrank_project_raw", "mix_nce", "mix_nce_raw", "mix_nce_workspace",
    "multinomial_nll", "multinomial_nll_raw", "multinomial_nll_workspace", "na_nce_loss", "na_nce_loss_raw",
    "na_nce_workspace", "ngcf_layer_tail", "ngcf_transform", "perturb_raw", "propagate_mean", "propagate_normalized",
    "propagate_views", "propagate_views_raw", "reg_rows_loss", "reg_rows_raw", "reset_noise_stream", "rows_chain_add_raw",
    "rows_chain_store2_raw", "rows_gather2_raw", "rows_gather_raw", "rows_layer_mean_raw", "rows_normalize",
    "rows_normalize_bwd_raw", "rows_normalize_raw", "rows_scatter_raw", "rows_tanh_bwd_raw", "sccf_loss", "sccf_loss_raw",
    "sccf_workspace", "score_dense", "score_topk", "score_topk_form", "side_stream", "spmm", "spmm_epi_raw", "spmm_ex_raw",
    "spmm_noise_raw", "spmm_perturbed", "spmm_rows_width", "subgraph_values_raw", "svd_nce_loss", "svd_nce_raw",
    "svd_nce_workspace", "table_nce_loss", "table_nce_raw", "table_nce_workspace", "tall_linear", "topk_option",
    "topk_options", "users_bitmap", "vae_head", "vae_head_bwd_raw", "vae_head_raw",
]
