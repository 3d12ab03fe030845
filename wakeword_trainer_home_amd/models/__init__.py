from .architectures import create_model, CNNSmallWakeword
from .lstm import LSTMWakeword
from .tcn import TCNWakeword
from .losses import create_loss_function, LabelSmoothingCrossEntropy, CrossEntropyLoss, FocalLoss

__all__ = ["create_model", "CNNSmallWakeword", "LSTMWakeword", "TCNWakeword", "create_loss_function", "LabelSmoothingCrossEntropy",
           "CrossEntropyLoss", "FocalLoss"]
