"""Host-side helpers of the reference's model/segment_anything/utils."""
