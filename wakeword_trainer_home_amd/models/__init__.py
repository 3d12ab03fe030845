from .architectures import create_model, CNNSmallWakeword
from .lstm import LSTMWakeword
from .tcn import TCNWakeword
from .resnet import ResNet18Wakeword
from .losses import create_loss_function, LabelSmoothingCrossEntropy, CrossEntropyLoss, FocalLoss

__all__ = ["create_model", "CNNSmallWakeword", "LSTMWakeword", "TCNWakeword", "ResNet18Wakeword", "create_loss_function",
           "LabelSmoothingCrossEntropy", "CrossEntropyLoss", "FocalLoss"]
