"""scaleprotoseg_amd — MI355X-native prototype-distance hot path of ScaleProtoSeg.

Public surface mirrors the reference's module/function names for this path:
    PPNetMultiScale, construct_PPNet                (segmentation/model/model_multiscale.py)
    PPNetMultiScaleGroup, construct_PPNet_Group     (segmentation/model/model_multiscale_group.py)
    PPNet                                           (segmentation/model/model.py, S = 1)
    compute_distances, min_across_dataset, global_min, push_prototypes_multiscale
                                                    (segmentation/push_multiscale_optimization.py)
    projection_simplex_sort, resize_label           (segmentation/utils.py, segmentation/data/dataset.py)
    projection_simplex_sort_                        (the same projection of all group projections IN PLACE, one launch,
                                                     bit-identical to the formula on the CPU; capturable)
    threshold_group_projections_, non_zero_proto    (segmentation/analysis/threshold_save.py:27-28, segmentation/utils.py:140-154:
                                                     zero the small group weights; the prototypes any group still uses)
    KLDLoss, KLDLossGroup                           (segmentation/model/loss.py; KLDLoss also takes the class-gathered
                                                     ClassDistances of forward_from_conv_features(target_labels=...))
    SegmentationMetrics                             (segmentation/eval_valid_multiscale.py:229-275: mIoU, per-class IoU,
                                                     pixel accuracy, nearest-prototype counts, top-k class purity,
                                                     counted on the GPU without full-resolution maps)
    find_k_nearest_patches_to_prototypes, prune_prototypes
                                                    (find_nearest.py, prune.py: k nearest training patches per prototype
                                                     and class-purity pruning, searched and merged on the GPU)
    EntropyGroup, CrossEntropyGroup, ScaleMax, GroupRegularizers, head_l1
                                                    (segmentation/model/loss.py:351-464 and the masked last-layer L1 of the
                                                     training modules: one forward and one backward launch, no host sync)
    EntropySpatLoss, EntropySamplLoss, NormLoss, ActivationRegularizers
                                                    (segmentation/model/loss.py:149-348: the activation-side terms over the
                                                     class-gathered planes, two reduction passes + one gradient pass)
    ActivationOverlap, high_activation_threshold    (segmentation/analysis/prototype_overlap.py, group_overlap.py: overlap
                                                     mIoU of the high-activation masks of one class's prototypes / groups;
                                                     cubic upsample + exact quantile threshold, recomputed, never stored)
    push_bounding_boxes, push_box_tables            (segmentation/push_multiscale_optimization.py:416-497, helpers.py:53-87:
                                                     the push's patch box and greedy high-activation crop per prototype)
    PushTable, push_single_pass                     (the same push in ONE pass over the data set, images encoded in batches:
                                                     running winners and their feature vectors kept on the GPU;
                                                     push_prototypes_multiscale(batch_size=...))
    ExplanationMaps, activation_heat_maps, dominant_slot_maps
                                                    (segmentation/analysis/sample_activations_prototype.py:71-133,
                                                     sample_activations_group.py:72-131: per-slot uint8 heat maps over a
                                                     class and the map of the dominant slot, one byte per pixel)
    nearest_images_to_prototypes, nearest_prototypes, high_activation_threshold_masked, patch_majority
                                                    (segmentation/analysis/nearest_img.py, nearest_proto.py: the n nearest
                                                     images of every prototype with the class-restricted threshold_gt and
                                                     both crops, and the n nearest prototypes of chosen pixels)
    FailureCases, predict_label_maps, failure_table, paired_heat_maps
                                                    (segmentation/analysis/failure_cases.py, segmentation/eval_test.py:99-111:
                                                     predicted label maps as bytes in the data set's ids with a confusion
                                                     matrix per image, the failing (image, class, mistaken-for) table, and
                                                     the two classes' heat maps over the failing class on shared ranges)
    scale_aggregate, WeightedAgg, OutSum, OutMult, OutConcat, factory_output_layer
                                                    (segmentation/model/scale_head.py, model_multiscale.py:306-314: a scale's
                                                     features combined with the activations of the scale above - the
                                                     scale_head_type of both PPNetMultiScale classes - as a pixel-tile
                                                     product on the fp32 matrix pipe, no [B, Pn, Cs, H, W] temporary)
    PartConsistency, PartStability, part_presence, part_thresholds, part_components
                                                    (segmentation/analysis/metrics/consistency.py, stability.py: which
                                                     prototypes or groups fire at the centroids of the annotated parts'
                                                     connected components; union-find labelling, weighted exact quantile)
    prepare_batch, resize_labels, draw_augmentation, BatchTable, fill_batch_table
                                                    (segmentation/data/dataset.py:143-186 and the per-step resize_label of
                                                     module_multiscale.py:234-236: the augmented, normalised window batch, its
                                                     labels and the latent labels of every grid from raw uint8 images, one launch)
    MSC, msc_max                                    (segmentation/utils.py:71-111: the backbone on the image and its shrunken
                                                     copies, the pixel-wise maximum of the bilinearly resampled outputs, the
                                                     add-on sigmoid and the bf16 cast in one launch;
                                                     ppnet.fuse_feature_epilogue() makes conv_features use it)
    msc_pack, PackedMaps, PackedLayout              (module_multiscale.py:216-277 runs the model on MSC's four training maps:
                                                     here they are written on one pixel axis in one launch, and one distance
                                                     forward / backward serves all four;
                                                     ppnet.fuse_feature_epilogue(dtype, packed=True))
    SegmentedCrossEntropy, segmented_cross_entropy  (module_multiscale_group_train.py:232-310: the cross entropy of every
                                                     segment of one packed forward, each with its own mean, counts and
                                                     gradient, in three launches without a host read; the group model takes a
                                                     PackedMaps too: PPNetMultiScaleGroup.forward_packed)
Arithmetic runs in libspx_hip.so (hand-written gfx950 HIP); there is no CPU fallback.
"""
from ._lib import SpxError, load as load_library  # noqa: F401
from .functional import (  # noqa: F401
    BankLayout,
    ClassGather,
    FusedCrossEntropy,
    SegmentedCE,
    cross_entropy_from_logits,
    segmented_cross_entropy,
    argmin_over_images,
    class_gather_table,
    proto_head_forward,
    decode_prune_keys,
    prune_footprint,
    prune_nearest_from_features,
    prune_nearest_from_map,
    push_masked_argmin,
    push_min_from_features,
    scale_aggregate,
    upsample_argext,
)
from .scale_head import OutConcat, OutMult, OutSum, WeightedAgg, factory_output_layer  # noqa: F401
from .msc import MSC, PackedLayout, PackedMaps, msc_max, msc_pack  # noqa: F401
from .checkpoint import export_state, import_state, load_reference_state_dict  # noqa: F401
from .loss import (  # noqa: F401
    ActivationRegularizers,
    ClassDistances,
    CrossEntropyGroup,
    EntropyGroup,
    EntropySamplLoss,
    EntropySpatLoss,
    GroupRegularizers,
    KLDLoss,
    KLDLossGroup,
    NormLoss,
    PixelWiseCrossEntropyLoss,
    ScaleMax,
    SegmentedCrossEntropy,
    head_l1,
)
from .metrics import SegmentationMetrics, SegmentationResult  # noqa: F401
from .model import PPNet  # noqa: F401
from .overlap import ActivationOverlap, OverlapResult, high_activation_threshold  # noqa: F401
from .model_multiscale import PPNetMultiScale, construct_PPNet  # noqa: F401
from .model_multiscale_group import PPNetMultiScaleGroup, construct_PPNet_Group  # noqa: F401
from .push import (  # noqa: F401
    PushTable,
    push_single_pass,
    compute_distances,
    global_min,
    min_across_dataset,
    push_box_tables,
    push_prototypes_multiscale,
)
from .pushbox import push_bounding_boxes  # noqa: F401
from .nearest import (  # noqa: F401
    NearestImages,
    high_activation_threshold_masked,
    nearest_images_to_prototypes,
    nearest_prototypes,
    patch_majority,
)
from .explain import ExplanationMaps, activation_heat_maps, dominant_slot_maps  # noqa: F401
from .failures import (  # noqa: F401
    BatchFailures,
    FailureCases,
    FailureReport,
    failure_table,
    paired_heat_maps,
    predict_label_maps,
)
from .parts import (  # noqa: F401
    PartComponents,
    PartConsistency,
    PartConsistencyResult,
    PartStability,
    PartStabilityResult,
    part_components,
    part_presence,
    part_thresholds,
)
from .batch import (  # noqa: F401
    AugmentParams,
    BatchTable,
    PreparedBatch,
    draw_augmentation,
    fill_batch_table,
    prepare_batch,
    resize_labels,
)
from .prune import NearestPatches, find_k_nearest_patches_to_prototypes, prune_prototypes  # noqa: F401
from .utils import (  # noqa: F401
    non_zero_proto,
    projection_simplex_sort,
    projection_simplex_sort_,
    resize_label,
    threshold_group_projections_,
)

__version__ = "0.1.0"
