"""``manner_amd.install()`` — bind the HIP operator classes INTO the reference's own package.

The reference selects its operators by Python import path: its LightningModules say
``from manner.models.components.news_encoder import MannerNewsEncoder`` (reference manner/models/cr_module.py:13-16,
a_module.py:15, ensemble_module.py:13, baselines/nrms_plm_module.py:15-16).  ``install()`` imports the REFERENCE's
``manner.models.components.{news_encoder, attention, user_encoder, click_predictors}`` modules as they are and replaces, inside
them, exactly the classes this build mirrors:

    news_encoder      MannerTextEncoder, MannerEntityEncoder, MannerNewsEncoder, PLMTextEncoder
    attention         AdditiveAttention
    user_encoder      NAMLUserEncoder, NRMSUserEncoder
    click_predictors  DotProduct

Everything else of those files — ``NAMLNewsEncoder``, ``LSTURNewsEncoder``, ``MINERNewsEncoder``, ``CAUMNewsEncoder``,
``PolyAttention``, ``TargetAwareAttention``, ``DenseAttention``, ``LSTURUserEncoder``, ``CAUMUserEncoder``, ``MINSUserEncoder`` —
stays the reference's own torch code by default (each has an opt-in below), and so do the names those classes captured at import time (the reference's
``NAMLNewsEncoder`` keeps using the reference's ``AdditiveAttention``: its module-level binding inside ``news_encoder`` is an import
of the ORIGINAL class object and is only replaced where it is one of the listed names of that module).  ``manner.utils``,
``manner.data``, ``manner.models.cr_module`` … are never touched: there is no ``manner`` package in this repository that could
shadow them (rounds 1-3 shipped a four-file shim package ``manner/``; it shadowed the reference tree and was removed).

Modules of the reference imported BEFORE ``install()`` (say ``manner.models.cr_module``, which has already executed its
``from … import MannerNewsEncoder``) are patched too: every module named ``manner`` / ``manner.*`` whose globals hold one of the
replaced class objects — under any alias, e.g. ``UserEncoder`` — is rebound, so the call order does not matter.

Opt-in baselines: ``install(baselines=("miner",))`` additionally rebinds the three leaf classes of the MINER baseline
(reference manner/models/baselines/miner_module.py:19-22 imports them as ``NewsEncoder``, ``UserEncoder`` and
``TargetAwareAttention``; its ``DotProduct`` is rebound already, and the mirror serves MINER's ``[B, C, D] x [B, D, K]`` call):

    news_encoder      MINERNewsEncoder
    attention         PolyAttention, TargetAwareAttention

``install(baselines=("caum_plm",))`` (the reference's config and module name, configs/model/caum_plm.yaml) rebinds the four leaf classes
of the CAUM baseline (baselines/caum_plm_module.py:15-16 imports ``CAUMNewsEncoder`` and ``CAUMUserEncoder``; they build the other two):

    news_encoder      CAUMCategoryEncoder, CAUMNewsEncoder
    user_encoder      CAUMUserEncoder
    attention         DenseAttention

``CAUMPLMModule``'s own lines — the per-candidate loop, ``to_dense_batch``, the loss, the metrics — stay the reference's torch
(``hotpath.caum_forward`` is its ``forward`` with the loop as one call, for a module that chooses to delegate: INTEGRATION §4).

``install(baselines=("lstur_plm",))`` (configs/model/lstur_plm.yaml; the experiments lstur_{ini,con}_{mind,adressa}) rebinds the three
leaf classes of the LSTUR baseline (baselines/lstur_plm_module.py imports ``LSTURNewsEncoder`` and ``LSTURUserEncoder``; the news
encoder builds the category encoder):

    news_encoder      LSTURCategoryEncoder, LSTURNewsEncoder
    user_encoder      LSTURUserEncoder

``LSTURPLMModule``'s own lines — ``to_dense_batch``, its Python loop for ``hist_size``, the loss, the metrics — stay the reference's
torch.

``install(baselines=("mins_plm",))`` (configs/model/mins_plm.yaml; the experiment mins_mind) rebinds the three leaf classes of the MINS
baseline (baselines/mins_plm_module.py imports ``NAMLNewsEncoder`` and ``MINSUserEncoder`` as ``NewsEncoder`` / ``UserEncoder``; the
news encoder builds the category encoder):

    news_encoder      NAMLCategoryEncoder, NAMLNewsEncoder
    user_encoder      MINSUserEncoder

``install(baselines=("naml_plm",))`` (configs/model/naml_plm.yaml; naml_mind) rebinds the two news-side classes alone — NAML-PLM's user
encoder, ``NAMLUserEncoder``, is bound by every install.  ``MINSPLMModule`` / ``NAMLPLMModule``'s own lines stay the reference's torch.

``MINERModule`` itself is not rebound, and the unchanged module keeps its torch lines; its category-bias construction, the max / mean
aggregation and the disagreement loss are built as ``hotpath.miner_forward`` / ``hotpath.miner_train_step`` (csrc/miner.hip) for a
``forward`` / ``model_step`` that delegates to them.  What stays the reference's torch: the metrics
bookkeeping of ``model_step`` and the Lightning hooks.  A plain ``install()`` binds exactly the first
table, whatever an earlier call added stays until ``uninstall()``.

``TANRPLMModule`` and ``SentiRecPLMModule`` have nothing to rebind and no baseline name: every leaf class of theirs —
``PLMTextEncoder``, ``NAMLUserEncoder`` / ``NRMSUserEncoder``, ``DotProduct`` — is in the first table.  Their own lines (the topic /
sentiment head over every news row, its loss, SentiRec's diversity regulariser) are built as ``hotpath.tanr_train_step`` and
``hotpath.sentirec_train_step`` (csrc/aspect.hip; ``tanr_forward`` / ``sentirec_forward`` beside them) for a ``forward`` /
``model_step`` that delegates to them.

``SentiDebiasPLMModule`` has nothing to rebind either (``PLMTextEncoder``, ``NRMSUserEncoder``, ``DotProduct``).  Its generator and
discriminator lines — the sentiment encoder as a class table, the orthogonality terms, the bias-aware scores, the adversarial
discriminator with its wrapped one-hot target — are built as ``hotpath.senti_debias_forward``, ``hotpath.senti_debias_generator_step``
and ``hotpath.senti_debias_discriminator_step`` (csrc/debias.hip) for a ``Generator.forward`` / ``training_step`` that delegates to
them; ``toggle_optimizer``, the two optimisers, the logging and the metrics stay the reference's.

``install(annotator=True)`` (a keyword of its own, default off) rebinds the data pipeline's ``SentimentAnnotator`` (reference
manner/data/components/sentiment_annotator.py) to ``manner_amd.data.components.sentiment_annotator.SentimentAnnotator`` in the three
modules that hold the name: ``manner.data.components.sentiment_annotator`` and ``mind_dataframe`` / ``adressa_dataframe``, which import
the class by name.  The mirror has no hub access: the frames' ``SentimentAnnotator(name, max_length)`` call then needs ``name`` to be
a local HF directory.  Nothing else of ``manner.data`` is touched.

``install(tsne=True)`` (a keyword of its own, default off) rebinds the name ``TSNE`` of ``manner.models.a_module`` — the reference's
``from MulticoreTSNE import MulticoreTSNE as TSNE`` (a_module.py:9), called by ``on_validation_epoch_end`` / ``on_test_epoch_end``
(a_module.py:150-173, 191-212) — to ``manner_amd.manifold.TSNE`` (csrc/tsne.hip: exact forces, ``angle`` ignored, not the package's bits).
Where the ``MulticoreTSNE`` package is not importable a shim module of that name, whose ``MulticoreTSNE`` attribute is the mirror, is
registered in ``sys.modules`` first, so that line 9 imports; ``uninstall()`` restores the name and removes the shim (an ``a_module`` that was
first imported through the shim never held another class: it keeps the mirror).  A plain ``install()`` touches neither.

Use (no reference source line changes):

    python -m manner_amd.run manner/train.py experiment=cr_module_mind_title_scl_lf      # = install() + runpy of the script
    python -m manner_amd.run --baselines miner manner/train.py experiment=miner_weighted_mind
    python -m manner_amd.run --baselines lstur_plm manner/train.py experiment=lstur_ini_mind
    python -m manner_amd.run --baselines mins_plm manner/train.py experiment=mins_mind

or two lines at the top of ``manner/train.py`` / ``manner/eval.py``:  ``import manner_amd; manner_amd.install()``.
"""
from __future__ import annotations

import importlib
import importlib.util
import sys
import types
from typing import Dict, List, Optional, Sequence, Tuple

TARGETS = {
    "news_encoder": ("MannerTextEncoder", "MannerEntityEncoder", "MannerNewsEncoder", "PLMTextEncoder"),
    "attention": ("AdditiveAttention",),
    "user_encoder": ("NAMLUserEncoder", "NRMSUserEncoder"),
    "click_predictors": ("DotProduct",),
}
BASELINE_TARGETS = {
    "miner": {"news_encoder": ("MINERNewsEncoder",), "attention": ("PolyAttention", "TargetAwareAttention")},
    "caum_plm": {"news_encoder": ("CAUMCategoryEncoder", "CAUMNewsEncoder"), "user_encoder": ("CAUMUserEncoder",),
                 "attention": ("DenseAttention",)},
    "lstur_plm": {"news_encoder": ("LSTURCategoryEncoder", "LSTURNewsEncoder"), "user_encoder": ("LSTURUserEncoder",)},
    "mins_plm": {"news_encoder": ("NAMLCategoryEncoder", "NAMLNewsEncoder"), "user_encoder": ("MINSUserEncoder",)},
    "naml_plm": {"news_encoder": ("NAMLCategoryEncoder", "NAMLNewsEncoder")},
}
_REF_PKG = "manner.models.components"
_MIRROR_PKG = "manner_amd.models.components"
_installed: Dict[str, Dict[str, type]] = {}          # module name -> {class name: the reference's original class}
ANNOTATOR_MODULES = ("manner.data.components.sentiment_annotator", "manner.data.components.mind_dataframe",
                     "manner.data.components.adressa_dataframe")


def _targets(baselines: Sequence[str]) -> Dict[str, Tuple[str, ...]]:
    if isinstance(baselines, str):
        baselines = (baselines,)
    unknown = [b for b in baselines if b not in BASELINE_TARGETS]
    if unknown:
        raise ValueError(f"manner_amd.install(): unknown baseline {unknown[0]!r} (known: {', '.join(sorted(BASELINE_TARGETS))})")
    targets = dict(TARGETS)
    for b in baselines:
        for leaf, names in BASELINE_TARGETS[b].items():
            targets[leaf] = targets.get(leaf, ()) + tuple(n for n in names if n not in targets.get(leaf, ()))
    return targets


def _install_annotator(report: Dict[str, List[str]]) -> None:
    from .data.components.sentiment_annotator import SentimentAnnotator as mirror
    for name in ANNOTATOR_MODULES:
        mod = importlib.import_module(name)
        cur = getattr(mod, "SentimentAnnotator")
        if cur is mirror:
            continue
        _installed.setdefault(name, {}).setdefault("SentimentAnnotator", cur)
        setattr(mod, "SentimentAnnotator", mirror)
        report.setdefault(name, []).append("SentimentAnnotator")


TSNE_MODULE, TSNE_PACKAGE = "manner.models.a_module", "MulticoreTSNE"
_tsne_shim: Optional[types.ModuleType] = None          # the stand-in registered as sys.modules["MulticoreTSNE"], if this module made one


def _install_tsne(report: Dict[str, List[str]]) -> None:
    global _tsne_shim
    from .manifold import TSNE as mirror
    real = None                                          # the package's class, where the package is there
    pkg = sys.modules.get(TSNE_PACKAGE)
    if pkg is None:
        try:
            found = importlib.util.find_spec(TSNE_PACKAGE) is not None
        except (ImportError, ValueError):
            found = False
        if found:
            pkg = importlib.import_module(TSNE_PACKAGE)
        else:
            pkg = types.ModuleType(TSNE_PACKAGE)
            pkg.__doc__ = "stand-in registered by manner_amd.install(tsne=True): MulticoreTSNE is manner_amd.manifold.TSNE"
            pkg.MulticoreTSNE = mirror
            sys.modules[TSNE_PACKAGE] = pkg
            _tsne_shim = pkg
    if pkg is not _tsne_shim:
        real = getattr(pkg, "MulticoreTSNE", None)
    mod = importlib.import_module(TSNE_MODULE)
    for attr, val in list(vars(mod).items()):
        if val is mirror:
            if attr == "TSNE" and _tsne_shim is not None and "TSNE" not in _installed.get(TSNE_MODULE, {}):
                # imported through the shim: the name was never anything else
                report.setdefault(TSNE_MODULE, []).append(attr)
            continue
        if (attr == "TSNE" and isinstance(val, type)) or (real is not None and val is real):
            _installed.setdefault(TSNE_MODULE, {}).setdefault(attr, val)
            setattr(mod, attr, mirror)
            report.setdefault(TSNE_MODULE, []).append(attr)


def install(reference_root: Optional[str] = None, baselines: Sequence[str] = (), annotator: bool = False,
            tsne: bool = False) -> Dict[str, List[str]]:
    """Rebind the mirrored classes inside the reference's ``manner.models.components`` modules.  ``reference_root``: a checkout
    of andreeaiana/manner to put on ``sys.path`` when ``manner`` is not importable yet.  ``baselines``: opt-in sets of further classes
    (``"miner"``: MINERNewsEncoder, PolyAttention, TargetAwareAttention; ``"caum_plm"``: CAUMCategoryEncoder, CAUMNewsEncoder,
    CAUMUserEncoder, DenseAttention; ``"lstur_plm"``: LSTURCategoryEncoder, LSTURNewsEncoder, LSTURUserEncoder; ``"mins_plm"``:
    NAMLCategoryEncoder, NAMLNewsEncoder, MINSUserEncoder; ``"naml_plm"``: NAMLCategoryEncoder, NAMLNewsEncoder); an unknown name raises
    ValueError.  ``annotator``: also rebind ``SentimentAnnotator`` in the reference's data components (off by default).  ``tsne``: also rebind
    ``manner.models.a_module.TSNE`` to ``manner_amd.manifold.TSNE``, behind a ``MulticoreTSNE`` shim module where that package is missing (off by
    default).  Returns {module: [rebound
    names]} (also the aliases patched in already-imported ``manner.*`` modules).  Idempotent; ``uninstall()`` restores the originals."""
    targets = _targets(baselines)
    if reference_root and reference_root not in sys.path:
        sys.path.insert(0, reference_root)
    report: Dict[str, List[str]] = {}
    swaps = {}                                       # id(original class) -> mirror class
    for leaf, names in targets.items():
        try:
            ref_mod = importlib.import_module(f"{_REF_PKG}.{leaf}")
        except ModuleNotFoundError as e:
            if (e.name or "").split(".")[0] == "manner":
                raise ModuleNotFoundError(
                    f"manner_amd.install(): the reference package `manner` is not importable ({e}); put a checkout of andreeaiana/manner on "
                    "PYTHONPATH or pass reference_root=") from e
            raise
        if getattr(ref_mod, "__file__", "").startswith(__file__.rsplit("/manner_amd/", 1)[0] + "/manner/"):
            raise RuntimeError("manner_amd.install(): `manner` resolves to a stale shim package inside this repository, not to the reference")
        mirror_mod = importlib.import_module(f"{_MIRROR_PKG}.{leaf}")
        kept = _installed.setdefault(ref_mod.__name__, {})
        for n in names:
            mirror = getattr(mirror_mod, n)
            cur = getattr(ref_mod, n)
            if cur is mirror:
                continue
            kept.setdefault(n, cur)
            swaps[id(cur)] = mirror
            setattr(ref_mod, n, mirror)
            report.setdefault(ref_mod.__name__, []).append(n)
    # aliases captured by reference modules that were imported before install(): patch by object identity
    if swaps:
        own = {f"{_REF_PKG}.{leaf}" for leaf in targets}
        for name, mod in list(sys.modules.items()):
            if mod is None or not (name == "manner" or name.startswith("manner.")) or name in own:
                continue
            for attr, val in list(vars(mod).items()):
                if isinstance(val, type) and id(val) in swaps:
                    _installed.setdefault(name, {}).setdefault(attr, val)
                    setattr(mod, attr, swaps[id(val)])
                    report.setdefault(name, []).append(attr)
    if annotator:
        _install_annotator(report)
    if tsne:
        _install_tsne(report)
    return report


def uninstall() -> None:
    """Put the reference's own classes back (tests)."""
    for modname, kept in _installed.items():
        mod = sys.modules.get(modname)
        if mod is not None:
            for n, orig in kept.items():
                setattr(mod, n, orig)
    _installed.clear()
    global _tsne_shim
    if _tsne_shim is not None:
        if sys.modules.get(TSNE_PACKAGE) is _tsne_shim:
            del sys.modules[TSNE_PACKAGE]
        _tsne_shim = None


def installed() -> Dict[str, List[str]]:
    out = {m: sorted(k) for m, k in _installed.items() if k}
    if _tsne_shim is not None:
        out[TSNE_PACKAGE] = ["MulticoreTSNE"]
        mod = sys.modules.get(TSNE_MODULE)
        if mod is not None and getattr(mod, "TSNE", None) is _tsne_shim.MulticoreTSNE and "TSNE" not in _installed.get(TSNE_MODULE, {}):
            out.setdefault(TSNE_MODULE, []).append("TSNE")
    return out
