from .architectures import create_model, CNNSmallWakeword
from .lstm import LSTMWakeword
from .losses import create_loss_function, LabelSmoothingCrossEntropy, CrossEntropyLoss, FocalLoss

__all__ = ["create_model", "CNNSmallWakeword", "LSTMWakeword", "create_loss_function", "LabelSmoothingCrossEntropy",
           "CrossEntropyLoss", "FocalLoss"]
