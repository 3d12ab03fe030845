"""Export: fp32 / fp16 / int8 bundles of a trained model, and the int8 ``cnn_small``, ``CRNNWakeword``, ``MobileNetV3Wakeword``,
``TCNWakeword``, ``ResNet18Wakeword`` and ``LSTMWakeword`` networks on the device (mirror of the reference's ``src/export/__init__.py``)."""
from .exporter import (BundleError, ExportConfig, ModelExporter, ONNXExporter, QuantizationError, QuantizedCNNSmall, QuantizedCRNN,
                       QuantizedLSTM, QuantizedMobileNetV3, QuantizedResNet18, QuantizedTCN, benchmark_exported_model, benchmark_onnx_model,
                       calibrate_cnn_small, calibrate_crnn, calibrate_lstm, calibrate_mobilenetv3, calibrate_resnet18, calibrate_tcn, export_model,
                       export_model_to_onnx, load_exported_model, validate_exported_model, validate_onnx_model)

__all__ = ["ExportConfig", "ModelExporter", "ONNXExporter", "export_model", "export_model_to_onnx", "load_exported_model",
           "validate_exported_model", "validate_onnx_model", "benchmark_exported_model", "benchmark_onnx_model",
           "QuantizedCNNSmall", "QuantizedTCN", "QuantizedResNet18", "QuantizedLSTM", "QuantizedCRNN", "BundleError",
           "QuantizationError", "calibrate_cnn_small", "calibrate_tcn", "calibrate_resnet18", "calibrate_lstm", "calibrate_crnn",
           "QuantizedMobileNetV3", "calibrate_mobilenetv3"]
