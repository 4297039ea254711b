"""The training loop of the `ml` module for one worker: MLConf (ml/conf/MLConf.scala:70-83) and
GeneralizedLinearModel with LRModel, SVMModel and LinearRegModel (ml/algorithm/*.scala), strung from the
pieces that run on the device: optim.miniBatchGradientDescent, gradient.compress, Gradient.sum's plusBy
and toAuto, Adam.update and validation.calLossPrecision.

train(), trainOneEpoch, trainOneIteration, computeGradient, aggregateAndUpdate and validate follow
GeneralizedLinearModel.scala:80-177 line by line with executors = one worker; what Spark aggregates over
workers is the worker's own value.  The caller passes trainData and validData: the reference's split
draws scala.util.Random inside a Spark partition and is not reproduced.  workerNum != 1 is refused; the
multi-rank loop over distributed.py is not built here.

Bit parity of the whole loop with the reference's arithmetic is claimed for compressor "None" and the
hinge and square losses; the log losses call the device's exp / log (within an ulp of Java's), and the
lossy compressors draw streams the reference leaves unseeded.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from .exceptions import SketchMLException
from .gradient import DenseDoubleGradient, Kind, compress
from .loss import L2HingeLoss, L2LogLoss, L2SquareLoss
from .optim import Adam
from .validation import calLossPrecision

ML_LOGISTIC_REGRESSION = "LogisticRegression"
ML_SUPPORT_VECTOR_MACHINE = "SupportVectorMachine"
ML_LINEAR_REGRESSION = "LinearRegression"
FORMATS = ("libsvm", "csv", "dummy")
COMPRESSORS = ("Sketch", "FixedPoint", "Zip", "Float", "None")


@dataclass
class MLConf:
    """case class MLConf with the defaults of object MLConf; algo, input, format, workerNum and
    featureNum have none there.  The three `require`s run at construction."""
    algo: str
    input: str
    format: str
    workerNum: int
    featureNum: int
    validRatio: float = 0.25
    epochNum: int = 100
    batchSpRatio: float = 0.1
    learnRate: float = 0.1
    learnDecay: float = 0.9
    l1Reg: float = 0.1
    l2Reg: float = 0.1
    compressor: str = "Sketch"
    quantBinNum: int = 256
    sketchGroupNum: int = 8
    sketchRowNum: int = 2
    sketchColRatio: float = 0.3
    fixedPointBitNum: int = 8

    def __post_init__(self):
        if self.algo not in (ML_LOGISTIC_REGRESSION, ML_SUPPORT_VECTOR_MACHINE, ML_LINEAR_REGRESSION):
            raise SketchMLException(f"Unsupported algorithm: {self.algo}")
        if self.format not in FORMATS:
            raise SketchMLException(f"Unrecognizable file format: {self.format}")
        if self.compressor not in COMPRESSORS:
            raise SketchMLException(f"Unrecognizable gradient compressor: {self.compressor}")

    def codec(self) -> dict:
        """What Gradient.compress reads from the configuration."""
        return {"quantBinNum": self.quantBinNum, "sketchGroupNum": self.sketchGroupNum, "sketchRowNum": self.sketchRowNum,
                "sketchColRatio": self.sketchColRatio, "fixedPointBitNum": self.fixedPointBitNum}


def gradient_sum(dim: int, grads, device) -> object:
    """Gradient.sum (Gradient.scala:44-49): a zero DenseDoubleGradient, plusBy of every gradient in order,
    toAuto.  plusBy adds a dense gradient's every value and a sparse one's values at their keys
    (DenseDoubleGradient.scala:35-57); the compressed kinds go through toDense / toSparse first."""
    total = torch.zeros(dim, dtype=torch.float64, device=device)
    for g in grads:
        if g.dim != dim:
            raise SketchMLException(f"a gradient of {g.dim} features in a sum of {dim}")
        if g.kind() not in (Kind.DenseDouble, Kind.SparseDouble):
            g = g.toAuto()
        if g.kind() == Kind.DenseDouble:
            total += g.values.to(torch.float64)
        else:
            total.index_add_(0, g.indices.long(), g.values.to(torch.float64))  # keys are distinct: one add each
    return DenseDoubleGradient(dim, total).toAuto()


class GeneralizedLinearModel:
    """abstract class GeneralizedLinearModel (GeneralizedLinearModel.scala:38-181) for one worker."""

    name = ""

    def __init__(self, conf: MLConf, trainData, validData, device=None, seed: int = 0, hashSeed: int = 0):
        if conf.workerNum != 1:
            raise SketchMLException(f"workerNum={conf.workerNum}: the multi-worker training loop is not built here "
                                    f"(DESIGN.md section 9); one worker trains on this device")
        self.conf, self.trainData, self.validData = conf, trainData, validData
        self.device = torch.device(device) if device is not None else trainData.device
        self.seed, self.hashSeed = int(seed), int(hashSeed)
        self.weights = self.optimizer = self.loss = self.gradient = None
        self.lastValidation = None

    # ---- initModel of the three models ----
    def _loss(self):
        raise NotImplementedError

    def initModel(self) -> None:
        c = self.conf
        self.weights = torch.zeros(c.featureNum, dtype=torch.float64, device=self.device)
        self.optimizer = Adam(c.featureNum, c.learnRate, c.learnDecay, c.batchSpRatio)
        self.loss = self._loss()

    def getName(self) -> str:
        return self.name

    # ---- GeneralizedLinearModel.scala:80-177 ----
    def train(self):
        """(trainLosses, validLosses, the last validation result).  The two lists are the ones the
        reference logs, which ArrayBuffer[Double](conf.epochNum) starts with epochNum as their first
        element (GeneralizedLinearModel.scala:86-87); the losses of the epochs follow."""
        self.initModel()
        trainLosses, validLosses = [float(self.conf.epochNum)], [float(self.conf.epochNum)]
        batchNum = int(math.ceil(1.0 / self.conf.batchSpRatio))
        for epoch in range(self.conf.epochNum):
            trainLosses.append(self.trainOneEpoch(epoch, batchNum))
            validLosses.append(self.validate(epoch))
        return trainLosses, validLosses, self.lastValidation

    def trainOneEpoch(self, epoch: int, batchNum: int) -> float:
        trainLoss = 0.0
        for batch in range(batchNum):
            trainLoss += self.trainOneIteration(epoch, batch)
        return trainLoss / batchNum

    def trainOneIteration(self, epoch: int, batch: int) -> float:
        batchLoss = self.computeGradient(epoch, batch)
        self.aggregateAndUpdate(epoch, batch)
        return batchLoss

    def computeGradient(self, epoch: int, batch: int) -> float:
        grad, batchSize, objLoss, regLoss = self.optimizer.miniBatchGradientDescent(self.weights, self.trainData, self.loss,
                                                                                    sequentialLoss=True)
        self.gradient = grad
        return objLoss / batchSize + regLoss / self.conf.workerNum

    def _compress(self, grad):
        return compress(grad, self.conf.compressor, seed=self.seed, hashSeed=self.hashSeed, **self.conf.codec())

    def aggregateAndUpdate(self, epoch: int, batch: int) -> None:
        total = gradient_sum(self.conf.featureNum, [self._compress(self.gradient)], self.device)
        grad = self._compress(total)
        grad.timesBy(1.0 / self.conf.workerNum)
        self.optimizer.update(grad, self.weights)

    def validate(self, epoch: int) -> float:
        self.lastValidation = calLossPrecision(self.weights, self.validData, self.loss)
        sumLoss, validNum = self.lastValidation[0], self.lastValidation[5]
        return sumLoss / validNum


class LRModel(GeneralizedLinearModel):
    """LRModel.scala:18-30: Adam over L2LogLoss(l2Reg)."""
    name = ML_LOGISTIC_REGRESSION

    def _loss(self):
        return L2LogLoss(self.conf.l2Reg)


class SVMModel(GeneralizedLinearModel):
    """SVMModel.scala:18-31: Adam over L2HingeLoss(l2Reg)."""
    name = ML_SUPPORT_VECTOR_MACHINE

    def _loss(self):
        return L2HingeLoss(self.conf.l2Reg)


class LinearRegModel(GeneralizedLinearModel):
    """LinearRegModel.scala:18-31: Adam over L2SquareLoss(l2Reg)."""
    name = ML_LINEAR_REGRESSION

    def _loss(self):
        return L2SquareLoss(self.conf.l2Reg)
