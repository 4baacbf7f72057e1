"""Torch-tensor front end of the C ABI (include/wdg.h): device CSR container + one Python function per kernel.

PyTorch is plumbing here (device memory, the current HIP stream); every computation below is a hand-written
gfx950 kernel in csrc/.  Nothing here runs on the CPU, and nothing falls back.

This module is the one namespace callers use (`from wdg_amd import ops`); the code lives in
  _rt.py                flag values of include/wdg.h, pointer helpers, the page-locked upload arena, the hipGraph capture harness
                        (capture_graphs, snapshot: TrainBatch, SplitTrainBatch and models.train_eval_graphed call it)
  graphs.py             CsrGraph (+ its one-time plans), GraphBatch (a shard's graphs in one build, or GENERATED on the device:
                        GraphBatch.generated), TwoHopBatch / two_hop (the strict two-hop neighbourhoods of a list of graphs as CsrGraphs:
                        two launches and one read-back), TopkRowsBatch / knn_graph / knn_graphs (the k best columns of every row of a
                        table of dense matrices in one launch; kNN feature graphs as CsrGraphs), normalisations
  synth.py              regular_graph_device, sample_feature_rows (the device generators; the numpy generators live there too),
                        class_graphs_device / ClassGraphBatch (classes of any sizes, a k and a d per class), gauss_features_device /
                        GaussFeatureBatch (Gaussian class features)
  csbmh.py              the CSBM-H closed forms (host, fp64), QdaBatch (the Bayes rule's error counts on x, A_rw x and x - A_rw x) and
                        empirical (the curves measured on sampled graphs); reached as wdg_amd.csbmh, not re-exported here
  aggregate.py          spmm, SpmmBatch (the quad-row kernel's tape and its cost cut), spmm_plan
  stats.py              edge / label statistics, LAS, per-edge cosine, their job tables
  gemm.py               gemm, gemm_skinny, GemmBatch, Mlp2Batch
  job_table.py          JobTable, StackedLogitsTable: what the job tables share (all but SpmmBatch, PropagatedGram and the builds) - the limit of one
                        launch, the buffers a table owns (offsets, byte strides, initial patterns, reset(), state_tensors()), the pointer
                        fill, the upload, the launch
  train.py              HeadTrainBatch (every epoch of many logistic heads in one launch), DropoutBatch (ReLU + counter-based
                        dropout of many hidden layers in one launch), AcmMixBatch (the channel mix of many ACM layers, forward and backward),
                        AcmMixPackedBatch (the same mix for stacked class-width layers: 1, 2 or 4 lanes per replica),
                        GatBatch (the graph-attention layer of many graphs, forward and backward: a softmax weight per stored entry),
                        GatScoresBatch (the scores of stacked attention layers, S = H blockdiag(a_dst, a_src) without the operand, forward and
                        backward with a parameter gradient summed in a stated order),
                        SignedAttBatch (the signed-attention layer of many graphs, forward and backward: a tanh weight per stored entry
                        times the fixed scales, an optional residual),
                        PolyFilterBatch (the polynomial graph filter sum_k gamma_k A_hat^k v of many graphs, all hops in one launch, with
                        the dot products that are the coefficients' gradient),
                        RecurFilterBatch (the same filter in a basis with a three-term recurrence - Chebyshev, Jacobi, Legendre - sum_k gamma_k T_k,
                        T_{k+1} = a_k A_hat T_k + b_k T_k + c_k T_{k-1}, all hops in one launch at the polynomial filter's row limits),
                        GcniiBatch (the GCNII layer behind its aggregation for many layers / graphs in one launch: initial residual, identity
                        mapping, ReLU + counter-based dropout, with a backward pass and a weight gradient summed in a stated order),
                        XentEvalBatch (cross-entropy gradient, hits and model selection of many models with stacked logits),
                        AdamBatch (the Adam step of a stacked run's parameter tensors in one launch: a learning rate and a weight
                        decay per replica in device memory, the step count read from the run's step word),
                        KeepBestBatch (the copy of every replica's parameters and logits at its best epoch, selected on the device),
                        ConfusionBatch (predictions and per-split confusion counts of stacked logits),
                        XentCurveBatch (the evaluation with losses: a learning curve, selection on validation loss, patience)
                        AucBatch (the exact ROC-AUC of stacked binary logits: selection on the validation AUC, patience, a curve)
  drop_edge.py          DropEdgeBatch (DropEdge: a fresh random subset of the stored entries of many graphs per step word in one launch, written
                        as thinned patterns - forward and transposed - with their renormalised scales), ThinnedSpmmBatch (the aggregation
                        over such patterns, one fmaf chain per element; its backward pass is the transposed pattern's job)
  neighbor_sample.py    NeighborSampleBatch (GraphSAGE's sampling: exactly `fanout` of every row's entries per step word, uniformly, written as
                        the same thinned patterns - the transposed one recomputed from one threshold word per forward row)
  neighbor_max.py       NeighborMaxBatch (the per-column maximum over every row's stored neighbours and which neighbour it was, over plain and
                        thinned patterns), NeighborMaxBackwardBatch (its backward pass: a job on the transposed pattern), neighbor_max
  neighbor_moments.py   NeighborMomentsBatch (PNA's four aggregators in one walk: per column the mean, the centred standard deviation, the
                        maximum and the minimum over every row's stored neighbours, the winners and the neighbour count, over plain and
                        thinned patterns), NeighborMomentsBackwardBatch (its backward pass: an elementwise launch and a job on the
                        transposed pattern inside one entry), neighbor_moments
  split_train.py        SplitTrainBatch (all splits of ONE graph trained as a single stacked run; reached as ops.SplitTrainBatch;
                        optimizer="device": per-replica lr / weight_decay / dropout), grid_search (a hyperparameter grid over all
                        splits as stacked chunks), select_settings
  acm_split_train.py    AcmSplitTrainBatch (all splits of ONE graph trained as a single stacked run of ACM-SGC-1 / ACM-GCN-2 models, in a
                        channel-major layout; reached as ops.AcmSplitTrainBatch)
  gat_split_train.py    GatSplitTrainBatch (all splits of ONE graph trained as a single stacked run of GAT-1 / GAT-2 models: the replicas'
                        layers are column-slice jobs of GatBatch, their scores one GatScoresBatch job per layer; reached as
                        ops.GatSplitTrainBatch)
  train_batch.py        TrainBatch (one model per graph of a shard, trained for all graphs at once; reached as sweep.TrainBatch)
  sparse_features.py    SparseFeatures (compact feature matrices on the host), expand_features / FeatureExpand (one launch for a list of them),
                        DeviceFeatures (a feature matrix on the device as CSR + its transposed index: matmul / t_matmul, the sparse first layer
                        of the stacked trainers), SparseDenseBatch (a table of such products)
  kernel_regression.py  GramBatch, PropagatedGram, RowRepBatch, EdgeGramBatch, KrSets, KrBatch, GnbBatch, SvmBatch
(module-level switches - aggregate.ABLATE_BITS, aggregate.NARROW_MIN_ENTRIES - are set on the module that owns them)."""
from ._lib import check, lib, require_gpu, stream_handle  # noqa: F401
from ._rt import (  # noqa: F401
    ACT_NONE, ACT_RELU, COO_ADD_SELF_LOOPS, COO_BINARISE, COO_DROP_SELF_LOOPS, COO_KEEP_DUPLICATES, COO_SYMMETRISE,
    GEMM_A_VEC4, NORM_RW, NORM_SYM, PREC_F32, PREC_F64, SPMM_ANY_COL_SCALE, SPMM_ANY_VAL, SPMM_DMA_OK,
    SPMM_HALF_SLAB, SPMM_SMALL_OFFSETS, Tiled, Transposed, _dev, _h2d, _H2D_MAX_BYTES, _ld, _PinnedArena, _ptr, _table,
)
from .graphs import (  # noqa: F401
    CsrGraph, degree_norm, GraphBatch, knn_graph, knn_graphs, normalise_values, quad_disabled, row_l1_normalise, row_rnorm, TopkRowsBatch,
    TOPK_EXCLUDE_SELF, TOPK_MAX_K, TOPK_SORT_COLUMNS, two_hop, two_hop_totals, TwoHopBatch, TWO_HOP_KEEP_ONE_HOP, TWO_HOP_KEEP_SELF,
    unpack_bits, _host_pack_coo,
)
from .aggregate import (  # noqa: F401
    QUAD_MULTI_ITEM_SU, spmm, spmm_plan, SpmmBatch, _dma_ok, _fill_job, _QUAD_COST_NS,
    _QUAD_COST_W, _quad_cut, _quad_segments, _quad_unit_cost, _quad_unit_costs, _sharing_groups,
)
from .stats import (  # noqa: F401
    edge_cosine, edge_label_stats, las, LasBatch, StatsBatch,
)
from .gemm import (  # noqa: F401
    gemm, gemm_skinny, GemmBatch, Mlp2Batch,
)
from .train import dropout_constants, AcmMixBatch, AcmMixPackedBatch, AdamBatch, AucBatch, ConfusionBatch, DropoutBatch, GatBatch, GatScoresBatch, GcniiBatch, HeadTrainBatch, KeepBestBatch, PolyFilterBatch, RecurFilterBatch, SignedAttBatch, XentCurveBatch, XentEvalBatch, AUC_RULE, SELECT_RULES, XENT_EVAL, XENT_GRAD  # noqa: F401
from .drop_edge import DropEdgeBatch, ThinnedPattern, ThinnedSpmmBatch, DROP_EDGE_KEEP_DIAGONAL, DROP_EDGE_NORM_SYM, DROP_EDGE_TIED, DROP_EDGE_TRANSPOSED  # noqa: F401
from .neighbor_sample import NeighborSampleBatch, NEIGHBOR_SAMPLE_KEEP_DIAGONAL, NEIGHBOR_SAMPLE_NORM_SYM, NEIGHBOR_SAMPLE_TRANSPOSED  # noqa: F401
from .neighbor_max import neighbor_max, NeighborMaxBackwardBatch, NeighborMaxBatch, NEIGHBOR_MAX_MIN  # noqa: F401
from .neighbor_moments import neighbor_moments, NeighborMomentsBackwardBatch, NeighborMomentsBatch  # noqa: F401
from .synth import class_graphs_device, ClassGraphBatch, gauss_features_device, GaussFeatureBatch, regular_graph_device, sample_feature_rows  # noqa: F401
from .sparse_features import as_compact, DeviceFeatures, expand_features, feature_image_floats, FeatureExpand, SparseDenseBatch, SparseFeatures  # noqa: F401
from .kernel_regression import (  # noqa: F401
    deflation_enabled, EdgeGramBatch, GnbBatch, GramBatch, kr_split_sizes, KrBatch, KrSets, PropagatedGram, RowRepBatch, SvmBatch, _KR_JOB_DTYPE,
)
from .split_train import classification_report, grid_search, masks_from_indices, prediction_overlap, random_masks, select_settings, SplitTrainBatch  # noqa: E402,F401  (last: it builds on the modules above)
from .acm_split_train import AcmSplitTrainBatch  # noqa: E402,F401
from .gat_split_train import GatSplitTrainBatch  # noqa: E402,F401
