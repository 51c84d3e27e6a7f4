"""Evaluation metrics of the reference's README ("Evaluation"): FID over SegmentEncoder features (fid.py), Contact Ratio (contact.py),
PSKL-J (psklj.py)."""
