"""MI355X-native radar point-cloud GNN (forward hot path of
UditBhaskar19/GRAPH_NEURAL_NETWORK_FOR_RADAR_PERCEPTION) on hand-written HIP kernels.

Drop-in entry points (same names / signatures as the reference):
  gnn_detector.Model_Inference, gnn_detector.Model_Training,
  gnn_detector.Model_Object_Classifier_Finetuning              (gnn_detector.py)
  loss.Loss_Graph, loss.Loss_Object_Class                      (loss.py)
  gnn_detector.Model_Inference_v2 (the GATv2 attention detector, forward only, fp32),
  gnn_attention.residual_graph_attn_block, graph_attention, GATv2Conv  (gnn_attention.py)
  gnn_blocks.*, common.*                                       (gnn_blocks.py, common.py)
  graph_features.compute_adjacency_information / _v2,
  compute_node_features, compute_edge_features                 (graph_features.py)
  config.config                                                (set_config_gnn.py)
  evaluation.compute_gt_and_pred_associations                  (detection_accuracy.py)
  objects.compute_proposals, objects.compute_cov_ellipse       (inference.py, ellipse.py)
Batched device path: graph_features.FrameBatch / build_graph_batch,
pipeline.RadarGNNPipeline.
Evaluation on the device (import from ``.evaluation``): evaluation.DetectionEvaluator
(performance_eval_detection.ipynb: confusion matrix, precision, recall) and
evaluation.SegmentationEvaluator (performance_eval_segmentation.ipynb).
A sequence on the device (import from ``.sequence``): sequence.SequenceStore holds a
RadarScenes sequence in HBM and cuts batches of sliding windows there (read_data.py's
get_sequence_data + extract_frame); evaluation.evaluate_sequence runs every window of a
sequence to the evaluators' count matrices.
Object stage on the device (import from ``.objects``): objects.object_list (process_frame's
numbers), objects.classifier_inputs (the classifier's training_data from the detector's
clusters) and objects.classify_proposals (detector -> classifier, no host loop).
"""
from . import config, synthetic  # noqa: F401

__version__ = '0.1.0'


def native_available() -> bool:
    """True when libradargnn.so is built and loads."""
    from . import _native
    try:
        _native.lib()
        return True
    except _native.NativeLibraryError:
        return False
