"""See tetranerf/utils/extension."""
