"""
ktf.io — Kaldi binary object readers (nnet3 raw models, PLDA models, vectors / matrices).

Host-side, one-time (weight loading). The public names and the data they return follow the
reference (kaldi_tflite/lib/io/kaldi/{object_reader,nnet3_reader,plda_reader,array_reader}.py:
`KaldiObjReader`, `KaldiNnet3Reader.{config,components,getWeights}`,
`KaldiPldaReader.{mean,transformMat,psi}`, `ReadKaldiArray`); the parser is not the reference's
token search. Kaldi's binary stream is self-delimiting --

    "<Tag> "                      a tag, followed by one of
    0x04 + 4 bytes | 0x08 + 8 bytes      a basic type (size byte + little-endian value)
    "T" | "F"                     a bool
    "FV "/"DV " + dim + data      a vector      (dim = 0x04 + int32)
    "FM "/"DM " + rows + cols + data     a matrix
    "FP "/"DP " + rows + data     a packed symmetric matrix
    text + " "                    a word (component name, ...)
    "<"                           nothing: the next tag

-- so an nnet3 file is decoded in ONE forward pass into (tag, payload) events (`iter_fields`), and a
component is the run of events between two <ComponentName> tags. `KaldiIvecExtractorReader` (io/kaldi/
ivector_extractor_reader.py) feeds ktf.layers.IvectorExtractor, together with `KaldiDiagGmmReader`, an extension of this
project for the diagonal UBM (`final.dubm`) of Kaldi's i-vector recipes.
"""

import re
import struct

import numpy as np

_I32 = struct.Struct("<i")
_F32 = struct.Struct("<f")
_F64 = struct.Struct("<d")
_CONTAINERS = {b"FV ": ("vec", np.float32), b"DV ": ("vec", np.float64), b"FM ": ("mat", np.float32),
               b"DM ": ("mat", np.float64), b"FP ": ("packed", np.float32), b"DP ": ("packed", np.float64)}

# 4-byte basic types are ambiguous on the wire (int32 or float32): the tags whose value is an integer
_INT_TAGS = {"<Dim>", "<BlockDim>", "<NumComponents>", "<RankIn>", "<RankOut>", "<UpdatePeriod>", "<InputDim>",
             "<OutputDim>", "<NumRepeats>", "<NumBlocks>"}
# tag -> key under which KaldiNnet3Reader stores the payload in a component dict (the reference's key names,
# nnet3_reader.py:189-225; other tags of a component are decoded and dropped)
_FIELD_KEYS = {
    "<Dim>": "dim", "<ValueAvg>": "value-avg", "<DerivAvg>": "deriv-avg", "<Count>": "count",
    "<OderivRms>": "oderiv-rms", "<OderivCount>": "oderiv-count",
    "<LinearParams>": "params", "<BiasParams>": "bias", "<Params>": "params",
    "<BlockDim>": "block-dim", "<Epsilon>": "epsilon", "<TargetRms>": "target-rms", "<TestMode>": "test-mode",
    "<StatsMean>": "stats-mean", "<StatsVar>": "stats-var",
}
# component kinds (type tag without "<", "Component>") whose fields are kept; anything else is rejected like the reference
_KINDS = {
    "Sigmoid": ("dim", "value-avg", "deriv-avg", "count", "oderiv-rms", "oderiv-count"),
    "Affine": ("params", "bias"),
    "Linear": ("params",),
    "BatchNorm": ("dim", "block-dim", "epsilon", "target-rms", "test-mode", "count", "stats-mean", "stats-var"),
    "StatisticsExtraction": (),
}
for _alias, _of in (("Tanh", "Sigmoid"), ("RectifiedLinear", "Sigmoid"), ("Softmax", "Sigmoid"), ("LogSoftmax", "Sigmoid"),
                    ("NoOp", "Sigmoid"), ("NaturalGradientAffine", "Affine"), ("StatisticsPooling", "StatisticsExtraction")):
    _KINDS[_alias] = _KINDS[_of]


class KaldiObjReader:
    """io/kaldi/object_reader.py:23 — a cursor (`curPos`) over the bytes of one Kaldi binary file with typed reads.
    Text-mode objects are not supported (NotImplementedError), as in the reference (:46-47)."""

    def __init__(self, path, binary):
        if not binary:
            raise NotImplementedError("objects in text format are currently not supported")
        self.path, self.binary, self.curPos = path, binary, 0
        with open(path, "rb") as f:
            self.data = f.read()

    # ---- raw bytes
    def _take(self, n):
        lo = self.curPos
        if lo + n > len(self.data):
            raise ValueError(f"{self.path}: truncated ({n} bytes wanted at offset {lo}, file has {len(self.data)})")
        self.curPos = lo + n
        return lo

    def readBytes(self, nBytes):
        lo = self.curPos
        self.curPos = min(len(self.data), lo + nBytes)
        return self.data[lo:self.curPos]

    def peekBytes(self, nBytes):
        return self.data[self.curPos:self.curPos + nBytes]

    def readLine(self):
        end = self.data.find(b"\n", self.curPos)
        if end < 0:
            raise ValueError("expected new line but did not get any")
        line = self.data[self.curPos:end].decode("utf-8", "replace")
        self.curPos = end + 1
        return line

    def expectLine(self):
        self.readLine()

    # ---- words and tags
    def readToken(self):
        end = self.data.find(b" ", self.curPos)
        if end < 0:
            raise ValueError(f"no whitespace separated token after pos {self.curPos}")
        word = self.data[self.curPos:end].decode("utf-8", "replace")
        self.curPos = end + 1
        return word

    def expectToken(self, token, stopTokens=()):
        """Moves the cursor just past the next occurrence of `token` (and the separator after it) and returns True; if
        one of `stopTokens` occurs earlier the cursor stays and the result is False (object_reader.py:147-196)."""
        want = token.encode()
        at = self.data.find(want, self.curPos)
        stops = [p for p in (self.data.find(s.encode(), self.curPos) for s in stopTokens) if p >= 0]
        if at >= 0 and not any(p < at for p in stops):
            self.curPos = at + len(want) + 1
            return True
        if stops:
            return False
        raise ValueError(f"failed to find expected token '{token}")

    # ---- basic types: one size byte, then the little-endian value
    def _basic(self, st):
        lo = self._take(1 + st.size)
        if self.data[lo] != st.size:
            raise ValueError(f"data type read is specified using {self.data[lo]} bytes, but want to parse {st.size} bytes")
        return st.unpack_from(self.data, lo + 1)[0]

    def readInt(self):
        return np.int32(self._basic(_I32))

    def readFloat(self):
        return np.float32(self._basic(_F32))

    def readDouble(self):
        return np.float64(self._basic(_F64))

    def readBasicType(self, dtype):
        return {4: self.readInt if np.issubdtype(dtype, np.integer) else self.readFloat, 8: self.readDouble}[np.dtype(dtype).itemsize]()

    def readBool(self):
        c = self.data[self._take(1):self.curPos]
        if c not in (b"T", b"F"):
            raise ValueError(f"unexpected format for booleans, expected 'T' or 'F', got {c}")
        return c == b"T"

    # ---- containers
    def _container(self, *kinds):
        head = bytes(self.peekBytes(3))
        if head[:2] == b"CM":
            raise NotImplementedError("can't decode compressed matrix yet")
        spec = _CONTAINERS.get(head)
        if spec is None or spec[0] not in kinds:
            raise ValueError(f"unknown header for {'/'.join(kinds)} type '{head}'")
        self.curPos += 3
        return spec[1]

    def _array(self, dtype, count):
        lo = self._take(count * np.dtype(dtype).itemsize)
        return np.frombuffer(self.data, dtype=dtype, count=count, offset=lo)

    def readVec(self):
        dtype = self._container("vec")
        return self._array(dtype, int(self.readInt()))

    def readMat(self):
        dtype = self._container("mat")
        rows, cols = int(self.readInt()), int(self.readInt())
        return self._array(dtype, rows * cols).reshape(rows, cols)

    def readPackedMat(self):
        """lower triangle, row by row -> full symmetric matrix (object_reader.py:434-483)."""
        dtype = self._container("packed")
        n = int(self.readInt())
        tri = self._array(dtype, n * (n + 1) // 2)
        full = np.zeros((n, n), dtype=dtype)
        r, c = np.tril_indices(n)
        full[r, c] = tri
        full[c, r] = tri
        return full

    # ---- one-pass event decoding
    def iter_fields(self, end_tag=None):
        """Yields (tag, payload) from the cursor on: payload is None (tag only), a word, a scalar, a bool or an array.
        Stops after `end_tag` (yielded with payload None) or at the end of the data."""
        data, n = self.data, len(self.data)
        while self.curPos < n:
            if data[self.curPos] in b" \n":
                self.curPos += 1
                continue
            if data[self.curPos] != 0x3C:           # not "<": a further value of the previous tag
                yield None, self._payload(None)
                continue
            tag = self.readToken()
            if tag == end_tag:
                yield tag, None
                return
            yield tag, self._payload(tag)

    def _payload(self, tag):
        head = bytes(self.peekBytes(3))
        if not head or head[:1] == b"<":
            return None
        if head[0] == 4:
            return self.readInt() if tag in _INT_TAGS else self.readFloat()
        if head[0] == 8:
            return self.readDouble()
        if head in _CONTAINERS:
            kind = _CONTAINERS[head][0]
            return {"vec": self.readVec, "mat": self.readMat, "packed": self.readPackedMat}[kind]()
        if head[:2] == b"CM":
            raise NotImplementedError("can't decode compressed matrix yet")
        if head[:1] in (b"T", b"F") and (len(head) == 1 or head[1:2] in (b"<", b" ")):
            return self.readBool()
        return self.readToken()


class KaldiNnet3Reader(KaldiObjReader):
    """io/kaldi/nnet3_reader.py:27 — `config`: the lines of the <Nnet3> header; `components`: one dict per component
    ({"name", "type", + the fields of nnet3_reader.py:189-225 that are present}) in file order."""

    def __init__(self, nnet3_path, binary):
        super().__init__(nnet3_path, binary)
        self.config, self.components = [], []
        self.read()

    def read(self):
        self.expectToken("<Nnet3>")
        if self.readLine().strip():
            raise ValueError("expected model config following <Nnet3> token, got blank line")
        self.config = []
        while True:
            line = self.readLine().strip()
            if not line:
                break
            self.config.append(line)
        self.components, cur, declared, closed = [], None, None, False
        for tag, val in self.iter_fields(end_tag="</Nnet3>"):
            if tag is None:
                continue
            if tag == "<NumComponents>":
                declared = int(val)
                assert 0 < declared < 100000, f"expected between 1 and 9999 components, got {declared}"
            elif tag == "<ComponentName>":
                cur = {"name": val, "type": None}
                self.components.append(cur)
            elif tag == "</Nnet3>":
                closed = True
            elif cur is not None and cur["type"] is None:
                cur["type"] = tag
                cur["_keep"] = _KINDS.get(self.stripTagsAndSuffix(tag, "Component"))
                if cur["_keep"] is None:
                    raise ValueError(f"unsupported component type '{tag}'")
                if val is not None:          # the type tag is followed directly by the first field's tag, never by data
                    raise ValueError(f"unexpected data after component type {tag}")
            elif cur is not None:
                key = _FIELD_KEYS.get(tag)
                if key in cur["_keep"] and key not in cur:
                    cur[key] = val
        if declared is None:
            raise ValueError("failed to find expected token '<NumComponents>")
        if not closed:
            raise ValueError("failed to find expected token '</Nnet3>")
        if len(self.components) != declared:
            raise ValueError(f"<NumComponents> says {declared}, file holds {len(self.components)}")
        for c in self.components:
            for key in c.pop("_keep"):
                if key not in c:
                    print(f"  - component {c['name']}: no field '{key}'")

    @staticmethod
    def stripTagsAndSuffix(token, suffix=""):
        """'<FooComponent>' -> 'Foo'."""
        core = token.strip("<>/")
        return core[:-len(suffix)] if suffix and core.endswith(suffix) else core

    def getComponent(self, name):
        """components whose name matches the regular expression `name` from its start (sequential.py:136-138 passes the
        layer name)."""
        pat = re.compile(name)
        return [c for c in self.components if pat.match(c["name"])]

    def getWeights(self, name):
        """[W (units, K*D), b] of an affine component, [target-rms, stats-mean, stats-var] of a batch-norm component,
        concatenated over every component matching `name`; KeyError when none does (nnet3_reader.py:316-324)."""
        found = self.getComponent(name)
        if not found:
            raise KeyError(f"no components with name matching '{name}'")
        order = {"NaturalGradientAffine": ("params", "bias"), "BatchNorm": ("target-rms", "stats-mean", "stats-var")}
        out = []
        for c in found:
            out += [c[k] for k in order.get(self.stripTagsAndSuffix(c["type"], "Component"), ())]
        return out


class KaldiPldaReader(KaldiObjReader):
    """io/kaldi/plda_reader.py:22 — <Plda> mean (dim), transformMat (dim, dim), psi (dim); float64 in Kaldi's files."""

    def __init__(self, plda_path, binary):
        super().__init__(plda_path, binary)
        self.read()

    def read(self):
        self.expectToken("<Plda>")
        self.mean, self.transformMat, self.psi = self.readVec(), self.readMat(), self.readVec()
        self.expectToken("</Plda>")


class KaldiIvecExtractorReader(KaldiObjReader):
    """io/kaldi/ivector_extractor_reader.py:26 — <IvectorExtractor> (I = numGauss Gaussians, D = featDim, S = ivecDim):
    w (I, S) or empty (ivector-dependent weights), wVec (I), M: I matrices (D, S), sigmaInv: I FULL symmetric (D, D) matrices,
    priorOffset; derived: sigmaInvM (I, D, S) = sigmaInv[i] @ M[i] and U (I, S(S+1)/2), the lower triangle of M[i]^T sigmaInvM[i]
    row by row. readPackedMat gives the full symmetric SigmaInv of a real extractor (the reference keeps only the lower triangle,
    which agrees on its diagonal dummies)."""

    def __init__(self, ivec_path, binary=True):
        super().__init__(ivec_path, binary)
        self.numGauss = self.featDim = self.ivecDim = None
        self.w = self.wVec = self.M = self.sigmaInv = self.priorOffset = self.U = self.sigmaInvM = None
        self.read()
        self.deriveVars()

    def read(self):
        self.expectToken("<IvectorExtractor>")
        self.expectToken("<w>")
        self.w = self.readMat()
        self.expectToken("<w_vec>")
        self.wVec = self.readVec()
        self.expectToken("<M>")
        self.numGauss = int(self.readInt())
        self.M = [self.readMat() for _ in range(self.numGauss)]
        self.expectToken("<SigmaInv>")
        self.sigmaInv = [self.readPackedMat() for _ in range(self.numGauss)]
        self.expectToken("<IvectorOffset>")
        self.priorOffset = self.readDouble()
        self.expectToken("</IvectorExtractor>")

    def deriveVars(self):
        if len(self.M) == 0:
            raise ValueError("expected at least 1 projection matrix (M_), got 0")
        self.featDim, self.ivecDim = int(self.M[0].shape[0]), int(self.M[0].shape[-1])
        if any(m.shape != (self.featDim, self.ivecDim) for m in self.M) or \
                any(s.shape != (self.featDim, self.featDim) for s in self.sigmaInv):
            raise ValueError("inconsistent M / SigmaInv shapes")
        self.sigmaInvM = np.matmul(self.sigmaInv, self.M)
        S = self.ivecDim
        r, c = np.tril_indices(S)
        self.U = np.zeros((self.numGauss, S * (S + 1) // 2), dtype=np.float64)
        for i0 in range(0, self.numGauss, 64):          # (64, S, S) at a time: a real extractor's full stack is GBs
            tmp = np.matmul(np.swapaxes(np.asarray(self.M[i0:i0 + 64]), 1, 2), self.sigmaInvM[i0:i0 + 64])
            self.U[i0:i0 + 64] = tmp[:, r, c]


class KaldiDiagGmmReader(KaldiObjReader):
    """Kaldi DiagGmm (`final.dubm`; an extension: the reference has no UBM reader): <DiagGMM> <GCONSTS> FV <WEIGHTS> FV
    <MEANS_INVVARS> FM <INV_VARS> FM </DiagGMM>. weights (I), means_invvars (I, D), inv_vars (I, D) as stored (fp32 in Kaldi's
    files); gconsts (I, fp32) are recomputed as DiagGmm::ComputeGconsts does,
    log w - D/2 log(2 pi) + sum_d (log iv_d / 2 - mi_d^2 / iv_d / 2) in fp32, and the stored ones are kept as `storedGconsts`."""

    def __init__(self, path, binary=True):
        super().__init__(path, binary)
        self.read()

    def read(self):
        self.expectToken("<DiagGMM>")
        self.storedGconsts = self.readVec() if self.expectToken("<GCONSTS>", stopTokens=("<WEIGHTS>",)) else None
        self.expectToken("<WEIGHTS>")
        self.weights = self.readVec()
        self.expectToken("<MEANS_INVVARS>")
        self.means_invvars = self.readMat()
        self.expectToken("<INV_VARS>")
        self.inv_vars = self.readMat()
        self.expectToken("</DiagGMM>")
        I, D = self.means_invvars.shape
        if self.inv_vars.shape != (I, D) or self.weights.shape != (I,) or I == 0:
            raise ValueError(f"inconsistent DiagGMM shapes: weights {self.weights.shape}, means_invvars {self.means_invvars.shape}, "
                             f"inv_vars {self.inv_vars.shape}")
        self.numGauss, self.featDim = int(I), int(D)
        self.gconsts = self.computeGconsts()

    def computeGconsts(self):
        """DiagGmm::ComputeGconsts with C++'s promotions: offset = BaseFloat(-0.5 * M_LOG_2PI * dim), gc = Log(w) + offset in
        fp32, then per dimension gc += 0.5 * Log(iv) - 0.5 * mi * mi / iv (the right side in double, gc rounded to fp32 each step)."""
        f = np.float32
        iv = self.inv_vars.astype(f)
        mi = self.means_invvars.astype(f).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            gc = np.log(self.weights.astype(f)) + f(-0.5 * np.log(2 * np.pi) * self.featDim)
            logiv = np.log(iv).astype(np.float64)                       # Log(float) is logf
            ivd = iv.astype(np.float64)
            for d in range(self.featDim):
                gc = (gc.astype(np.float64) + (0.5 * logiv[:, d] - 0.5 * mi[:, d] * mi[:, d] / ivd[:, d])).astype(f)
        return gc.astype(f)


class KaldiFullGmmReader(KaldiObjReader):
    """Kaldi FullGmm (`final.ubm`; an extension like KaldiDiagGmmReader): <FullGMM> <GCONSTS> FV <WEIGHTS> FV <MEANS_INVCOVARS> FM
    <INV_COVARS> (FP) x I </FullGMM>, the I packed lower triangles following each other without a count, fp32. weights (I),
    means_invcovars (I, D) as stored, inv_covars (I, D, D) full symmetric fp32; <GCONSTS> may be absent (`storedGconsts` None).
    gconsts (I, fp32) are recomputed as FullGmm::ComputeGconsts defines them, log w - D/2 log(2 pi) - (log det Sigma + mu^T
    Sigma^-1 mu) / 2, in fp64 from the stored fp32 fields and rounded once to fp32: Kaldi's own promotions inside ComputeGconsts are
    not known to this project, so the last bit may differ from the stored values. A non-positive-definite inv_covars[i] or
    inconsistent shapes raise ValueError."""

    def __init__(self, path, binary=True):
        super().__init__(path, binary)
        self.read()

    def read(self):
        self.expectToken("<FullGMM>")
        self.storedGconsts = self.readVec() if self.expectToken("<GCONSTS>", stopTokens=("<WEIGHTS>",)) else None
        self.expectToken("<WEIGHTS>")
        self.weights = self.readVec()
        self.expectToken("<MEANS_INVCOVARS>")
        self.means_invcovars = self.readMat()
        self.expectToken("<INV_COVARS>")
        I, D = self.means_invcovars.shape
        if self.weights.shape != (I,) or I == 0 or D == 0:
            raise ValueError(f"inconsistent FullGMM shapes: weights {self.weights.shape}, means_invcovars {self.means_invcovars.shape}")
        covs = []
        for i in range(I):
            covs.append(self.readPackedMat())
            if covs[-1].shape != (D, D):
                raise ValueError(f"inconsistent FullGMM shapes: inv_covars[{i}] is {covs[-1].shape}, feature dim {D}")
        self.expectToken("</FullGMM>")
        self.inv_covars = np.asarray(covs, dtype=np.float32)
        self.numGauss, self.featDim = int(I), int(D)
        self.gconsts = self.computeGconsts()

    def _covars(self):
        """(Sigma (I, D, D), log det Sigma (I)) in fp64; ValueError if an inverse covariance is not positive definite."""
        ic = self.inv_covars.astype(np.float64)
        try:
            chol = np.linalg.cholesky(ic)
        except np.linalg.LinAlgError as e:
            raise ValueError(f"FullGMM: an inverse covariance is not positive definite ({e})") from None
        if not np.isfinite(chol).all():
            raise ValueError("FullGMM: an inverse covariance is not positive definite")
        logdet = -2.0 * np.log(np.diagonal(chol, axis1=1, axis2=2)).sum(1)
        return np.linalg.inv(ic), logdet

    def computeGconsts(self):
        cov, logdet = self._covars()
        mic = self.means_invcovars.astype(np.float64)
        mu = np.einsum("ide,ie->id", cov, mic)
        with np.errstate(divide="ignore"):
            gc = np.log(self.weights.astype(np.float64)) - 0.5 * self.featDim * np.log(2 * np.pi) \
                - 0.5 * (logdet + np.einsum("id,id->i", mu, mic))
        return gc.astype(np.float32)

    def toDiag(self):
        """fgmm-global-to-gmm (DiagGmm::CopyFromFullGmm): Sigma = inv(inv_covars) in fp64, inv_vars = 1 / diag Sigma, means_invvars
        = (Sigma means_invcovars) inv_vars, the same weights -> an object with KaldiDiagGmmReader's attributes."""
        cov, _ = self._covars()
        iv = 1.0 / np.diagonal(cov, axis1=1, axis2=2)
        mu = np.einsum("ide,ie->id", cov, self.means_invcovars.astype(np.float64))
        d = KaldiDiagGmmReader.__new__(KaldiDiagGmmReader)
        d.path, d.binary, d.storedGconsts = self.path, True, None
        d.weights = np.array(self.weights, dtype=np.float32)
        d.inv_vars = iv.astype(np.float32)
        d.means_invvars = (mu * iv).astype(np.float32)
        d.numGauss, d.featDim = self.numGauss, self.featDim
        d.gconsts = d.computeGconsts()
        return d


def _text_array(path, dtype):
    """Kaldi text form: ' [ v v v ]' on one line is a vector; '[' ... rows ... ']' over several lines a matrix."""
    if dtype not in (np.float32, np.float64, np.int16, np.int32, np.int64):
        raise ValueError(f"unsupported data type: {dtype}")
    parse = np.float64 if np.issubdtype(dtype, np.floating) else np.int64
    with open(path, "r") as f:
        text = f.read()
    lo, hi = text.find("["), text.find("]")
    if lo < 0 or hi < lo:
        raise ValueError("reached end of file without finding closing bracket for matrix")
    body = text[lo + 1:hi]
    if "\n" not in body:
        return np.array(body.split(), dtype=parse).astype(dtype)
    rows = [np.array(r.split(), dtype=parse) for r in body.split("\n") if r.strip()]
    return np.array(rows).astype(dtype) if rows else np.zeros((0, 0), dtype=dtype)


def ReadKaldiArray(path, binary, dtype=np.float32):
    """io/kaldi/array_reader.py:24 — one vector or matrix from a binary ("\\0B" + FV/DV/FM/DM) or text ([ ... ]) file."""
    if not binary:
        return _text_array(path, dtype)
    r = KaldiObjReader(path, True)
    r.curPos = 2                                   # "\0B"
    kind = bytes(r.peekBytes(2))
    if kind in (b"FM", b"DM", b"CM"):
        return r.readMat()
    if kind in (b"FV", b"DV"):
        return r.readVec()
    raise ValueError(f"binary file contains unexpected header bytes, {kind.decode(errors='replace')}, expected 'FV', 'DV', 'FM', 'DM' or 'CM'")


# ----------------------------------------------------------------------------- writers (an extension: the reference only reads)
def _array_bytes(array, binary):
    """One Kaldi vector / matrix as it follows "\\0B" or a token: binary "FV " / "DV " / "FM " / "DM ", then 0x04 + int32 sizes,
    then the little-endian data; text " [ v v v ]\\n" (vector) or " [" + "\\n  v v v " per row + "]\\n" (matrix), fp32 values as
    '%.7g', fp64 values as '%.17g' (exact on reading back)."""
    a = np.asarray(array)
    if a.dtype not in (np.float32, np.float64) or a.ndim not in (1, 2):
        raise ValueError(f"expected a float32 / float64 vector or matrix, got {a.dtype} of shape {a.shape}")
    f32 = a.dtype == np.float32
    if binary:
        head = (b"F" if f32 else b"D") + (b"V " if a.ndim == 1 else b"M ")
        sizes = b"".join(b"\x04" + _I32.pack(int(n)) for n in a.shape)
        return head + sizes + np.ascontiguousarray(a, dtype="<f4" if f32 else "<f8").tobytes()
    fmt = "%.7g" if f32 else "%.17g"
    if a.ndim == 1:
        return (" [ " + "".join(fmt % v + " " for v in a) + "]\n").encode()
    return (" [" + "".join("\n  " + "".join(fmt % v + " " for v in row) for row in a) + "]\n").encode()


def WriteKaldiArray(path, array, binary=True):
    """The inverse of ReadKaldiArray: a vector or matrix, fp32 -> FV / FM, fp64 -> DV / DM; binary files start with "\\0B"."""
    with open(path, "wb") as f:
        f.write((b"\0B" if binary else b"") + _array_bytes(array, binary))


def WriteKaldiPlda(path, mean, transform, psi, binary=True):
    """Kaldi's Plda::Write: "<Plda> ", mean (DV), transform (DM), psi (DV), "</Plda> " (binary: after "\\0B"). The arrays are
    written as fp64 whatever their dtype."""
    mean, transform, psi = (np.asarray(a, np.float64) for a in (mean, transform, psi))
    D = mean.shape[0]
    if mean.ndim != 1 or transform.shape != (D, D) or psi.shape != (D,):
        raise ValueError(f"inconsistent PLDA shapes: mean {mean.shape}, transform {transform.shape}, psi {psi.shape}")
    with open(path, "wb") as f:
        f.write((b"\0B" if binary else b"") + b"<Plda> " + _array_bytes(mean, binary) + _array_bytes(transform, binary)
                + _array_bytes(psi, binary) + b"</Plda> ")


class IvecExtractorModel(KaldiIvecExtractorReader):
    """An i-vector extractor held in memory (training.ivector_extractor_init / ivector_extractor_est), usable wherever a
    KaldiIvecExtractorReader is: M (I, D, S), sigmaInv (I, D, D) full symmetric, priorOffset, wVec (I; default: the log of uniform
    weights), w (default: empty, no ivector-dependent weights), all fp64; sigmaInvM and U are derived as the reader derives them."""

    def __init__(self, M, sigmaInv, priorOffset, wVec=None, w=None):
        M = np.ascontiguousarray(M, dtype=np.float64)
        sig = np.ascontiguousarray(sigmaInv, dtype=np.float64)
        if M.ndim != 3 or sig.shape != (M.shape[0], M.shape[1], M.shape[1]) or M.shape[0] < 1:
            raise ValueError(f"inconsistent extractor shapes: M {M.shape}, sigmaInv {sig.shape}")
        self.path, self.binary = None, True
        self.numGauss = int(M.shape[0])
        self.M, self.sigmaInv = list(M), list(sig)
        self.priorOffset = float(priorOffset)
        self.wVec = np.full(self.numGauss, -np.log(self.numGauss)) if wVec is None else np.asarray(wVec, np.float64)
        self.w = np.zeros((0, 0), np.float64) if w is None else np.asarray(w, np.float64)
        if self.wVec.shape != (self.numGauss,):
            raise ValueError(f"wVec must hold {self.numGauss} values, got {self.wVec.shape}")
        self.deriveVars()


def _packed_bytes(a):
    """One symmetric fp64 matrix as Kaldi's SpMatrix<double>: "DP ", 0x04 + int32 rows, the lower triangle row by row."""
    a = np.asarray(a, np.float64)
    n = a.shape[0]
    if a.shape != (n, n):
        raise ValueError(f"expected a square matrix, got {a.shape}")
    return b"DP " + b"\x04" + _I32.pack(n) + np.ascontiguousarray(a[np.tril_indices(n)], dtype="<f8").tobytes()


def WriteKaldiIvecExtractor(path, extractor, binary=True):
    """Kaldi's IvectorExtractor::Write, binary mode: "\\0B<IvectorExtractor> <w> " DM "<w_vec> " DV "<M> " int32 I, I x DM,
    "<SigmaInv> " I x DP (packed fp64 lower triangles) "<IvectorOffset> " double "</IvectorExtractor> ". `extractor`: a
    KaldiIvecExtractorReader or IvecExtractorModel. Everything is written as fp64; text mode is not implemented."""
    if not binary:
        raise NotImplementedError("WriteKaldiIvecExtractor writes Kaldi's binary mode only")
    e = extractor
    I = int(e.numGauss)
    if len(e.M) != I or len(e.sigmaInv) != I:
        raise ValueError("inconsistent extractor: numGauss does not match M / sigmaInv")
    w = np.asarray(e.w, np.float64)
    w = w if w.ndim == 2 else np.zeros((0, 0), np.float64)
    out = [b"\0B<IvectorExtractor> <w> ", _array_bytes(w, True), b"<w_vec> ", _array_bytes(np.asarray(e.wVec, np.float64).reshape(-1), True),
           b"<M> \x04", _I32.pack(I)]
    out += [_array_bytes(np.asarray(m, np.float64), True) for m in e.M]
    out.append(b"<SigmaInv> ")
    out += [_packed_bytes(s) for s in e.sigmaInv]
    out += [b"<IvectorOffset> \x08", struct.pack("<d", float(e.priorOffset)), b"</IvectorExtractor> "]
    with open(path, "wb") as f:
        f.write(b"".join(out))


class DiagGmmModel(KaldiDiagGmmReader):
    """A diagonal GMM held in memory (training.init_diag_ubm / diag_gmm_est), usable wherever a KaldiDiagGmmReader is: weights (I),
    means_invvars (I, D), inv_vars (I, D), rounded once to fp32 as Kaldi stores them; gconsts by the reader's computeGconsts."""

    def __init__(self, weights, means_invvars, inv_vars):
        w, mi, iv = (np.ascontiguousarray(a, dtype=np.float32) for a in (weights, means_invvars, inv_vars))
        if mi.ndim != 2 or iv.shape != mi.shape or w.shape != (mi.shape[0],) or mi.shape[0] < 1 or mi.shape[1] < 1:
            raise ValueError(f"inconsistent DiagGMM shapes: weights {w.shape}, means_invvars {mi.shape}, inv_vars {iv.shape}")
        self.path, self.binary, self.storedGconsts = None, True, None
        self.weights, self.means_invvars, self.inv_vars = w, mi, iv
        self.numGauss, self.featDim = int(mi.shape[0]), int(mi.shape[1])
        self.gconsts = self.computeGconsts()


class FullGmmModel(KaldiFullGmmReader):
    """A full-covariance GMM held in memory (training.diag_to_full / full_gmm_est), usable wherever a KaldiFullGmmReader is: weights
    (I), means_invcovars (I, D), inv_covars (I, D, D), rounded once to fp32; the lower triangle of every inverse covariance is
    mirrored (Kaldi stores that triangle alone), so inv_covars is symmetric bit for bit. gconsts by the reader's computeGconsts,
    which raises ValueError if an inverse covariance is not positive definite."""

    def __init__(self, weights, means_invcovars, inv_covars):
        w, mic = (np.ascontiguousarray(a, dtype=np.float32) for a in (weights, means_invcovars))
        ic = np.array(inv_covars, dtype=np.float32)
        if mic.ndim != 2 or ic.shape != mic.shape + mic.shape[1:] or w.shape != (mic.shape[0],) or mic.shape[0] < 1 or mic.shape[1] < 1:
            raise ValueError(f"inconsistent FullGMM shapes: weights {w.shape}, means_invcovars {mic.shape}, inv_covars {ic.shape}")
        r, c = np.tril_indices(mic.shape[1])
        ic[:, c, r] = ic[:, r, c]
        self.path, self.binary, self.storedGconsts = None, True, None
        self.weights, self.means_invcovars, self.inv_covars = w, mic, ic
        self.numGauss, self.featDim = int(mic.shape[0]), int(mic.shape[1])
        self.gconsts = self.computeGconsts()


def WriteKaldiDiagGmm(path, gmm, binary=True):
    """Kaldi's DiagGmm::Write, binary mode: "\\0B<DiagGMM> <GCONSTS> " FV "<WEIGHTS> " FV "<MEANS_INVVARS> " FM "<INV_VARS> " FM
    "</DiagGMM> ", all fp32. `gmm`: a KaldiDiagGmmReader or DiagGmmModel; the gconsts written are gmm.gconsts. Text mode is not
    implemented."""
    if not binary:
        raise NotImplementedError("WriteKaldiDiagGmm writes Kaldi's binary mode only")
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    I, D = f32(gmm.means_invvars).shape
    if f32(gmm.inv_vars).shape != (I, D) or f32(gmm.weights).shape != (I,) or f32(gmm.gconsts).shape != (I,):
        raise ValueError("inconsistent DiagGMM shapes")
    with open(path, "wb") as f:
        f.write(b"\0B<DiagGMM> <GCONSTS> " + _array_bytes(f32(gmm.gconsts), True) + b"<WEIGHTS> " + _array_bytes(f32(gmm.weights), True)
                + b"<MEANS_INVVARS> " + _array_bytes(f32(gmm.means_invvars), True) + b"<INV_VARS> " + _array_bytes(f32(gmm.inv_vars), True)
                + b"</DiagGMM> ")


def WriteKaldiFullGmm(path, gmm, binary=True):
    """Kaldi's FullGmm::Write, binary mode: "\\0B<FullGMM> <GCONSTS> " FV "<WEIGHTS> " FV "<MEANS_INVCOVARS> " FM "<INV_COVARS> " then
    I packed fp32 lower triangles ("FP ", 0x04 + int32 rows, the triangle row by row) "</FullGMM> ". `gmm`: a KaldiFullGmmReader or
    FullGmmModel. Text mode is not implemented."""
    if not binary:
        raise NotImplementedError("WriteKaldiFullGmm writes Kaldi's binary mode only")
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    I, D = f32(gmm.means_invcovars).shape
    ic = f32(gmm.inv_covars)
    if ic.shape != (I, D, D) or f32(gmm.weights).shape != (I,) or f32(gmm.gconsts).shape != (I,):
        raise ValueError("inconsistent FullGMM shapes")
    r, c = np.tril_indices(D)
    out = [b"\0B<FullGMM> <GCONSTS> ", _array_bytes(f32(gmm.gconsts), True), b"<WEIGHTS> ", _array_bytes(f32(gmm.weights), True),
           b"<MEANS_INVCOVARS> ", _array_bytes(f32(gmm.means_invcovars), True), b"<INV_COVARS> "]
    out += [b"FP \x04" + _I32.pack(D) + np.ascontiguousarray(ic[i][r, c], dtype="<f4").tobytes() for i in range(I)]
    out.append(b"</FullGMM> ")
    with open(path, "wb") as f:
        f.write(b"".join(out))
