// Stand-in message struct (TEST INFRASTRUCTURE ONLY; see ../ros/ros.h). Field types as in the
// message definition: float32 angles and ranges.
#ifndef F110_REFSHIM_LASERSCAN_H
#define F110_REFSHIM_LASERSCAN_H
#include <memory>
#include <vector>
namespace sensor_msgs {
struct LaserScan {
  typedef std::shared_ptr<const LaserScan> ConstPtr;
  float angle_min = 0, angle_max = 0, angle_increment = 0;
  float time_increment = 0, scan_time = 0, range_min = 0, range_max = 0;
  std::vector<float> ranges, intensities;
};
}
#endif
