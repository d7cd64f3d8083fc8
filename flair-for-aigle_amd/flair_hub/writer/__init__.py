"""Test stage: prediction rasters, confusion matrices and metrics.json (the reference's flair_hub/writer)."""
