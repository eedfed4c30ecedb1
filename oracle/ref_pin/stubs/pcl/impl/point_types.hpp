// pcl/impl/point_types.hpp for the reference pin: the reference's Volume.hpp and
// OccupancyGrid.hpp include it by name; the point types come from dmf_types.hpp.
#pragma once
