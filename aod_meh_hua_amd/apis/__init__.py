from .test import (BADGE_uncertainty, KMeansPP_uncertainty, single_gpu_badge_embeddings,
                   CCMS_uncertainty, CDAL_uncertainty, Consistency_uncertainty, Coreset_uncertainty, DivProto_uncertainty, ENMS_uncertainty,
                   Ensemble_uncertainty,
                   LocStability_uncertainty, MCDropout_uncertainty, Posterior_uncertainty, calculate_uncertainty,
                   single_gpu_cdal_descriptors, single_gpu_coco_map, single_gpu_consistency, single_gpu_descriptors, single_gpu_enms,
                   single_gpu_ensemble, single_gpu_loc_stability, single_gpu_mcdropout, single_gpu_object_descriptors, single_gpu_test, single_gpu_uncertainty,
                   sync_class_difficulty)
from .train_Lambda import train_detector_SSL

__all__ = ['BADGE_uncertainty', 'KMeansPP_uncertainty', 'single_gpu_badge_embeddings',
           'CCMS_uncertainty', 'CDAL_uncertainty', 'Consistency_uncertainty', 'Coreset_uncertainty', 'DivProto_uncertainty', 'ENMS_uncertainty',
           'Ensemble_uncertainty',
           'LocStability_uncertainty', 'MCDropout_uncertainty', 'Posterior_uncertainty', 'calculate_uncertainty',
           'single_gpu_cdal_descriptors', 'single_gpu_coco_map', 'single_gpu_consistency', 'single_gpu_descriptors', 'single_gpu_enms', 'single_gpu_ensemble',
           'single_gpu_loc_stability', 'single_gpu_mcdropout', 'single_gpu_object_descriptors', 'single_gpu_test', 'single_gpu_uncertainty',
           'sync_class_difficulty', 'train_detector_SSL']
