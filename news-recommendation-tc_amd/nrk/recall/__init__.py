"""The recall plugins, under the names src/recall/__init__.py exports."""
from .base import BaseRecaller
from .coldstart_recaller import ColdStartRecaller
from .fusion import RecallEnsemble, RecallFusion
from .itemcf_recaller import ItemCFRecaller
from .usercf_recaller import UserCFRecaller
from .youtubednn_recaller import YoutubeDNNRecaller

__all__ = ["BaseRecaller", "ItemCFRecaller", "UserCFRecaller", "YoutubeDNNRecaller", "ColdStartRecaller",
           "RecallFusion", "RecallEnsemble"]
